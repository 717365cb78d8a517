"""One rank of the multi-process wide-key render test (tests/test_gpu_wide_render.py): counts its shard of a seeded
wide-key workload (test_gpu_wide_keys._build) on device 0, joins the job's exchange (bc_comm_create_host +
bc_engine_finish_all), and on the root writes the text of the job's counts (bc_engine_render_wide_counts per sample,
bc_engine_render_wide_merged with the samples in descending order) as JSON.
    python tests/mp_rank_wide_render.py <rank> <world> <comm-dir> <n-total> <root> <out.json> <case>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    rank, world, cdir, n_total, root, out, name = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]),
                                                   int(sys.argv[5]), sys.argv[6], sys.argv[7])
    import torch  # noqa: F401 -- before the engine library: one HIP runtime in the process
    import ngs_barcode_count_amd as pkg
    import test_gpu_wide_keys as wk
    plan, _, reads = wk._build(name, n_total, 7)
    a, b = n_total * rank // world, n_total * (rank + 1) // world
    eng, _ = wk._run_engine(plan, reads[a:b], trace=False)
    comm = pkg.Comm.host(cdir, rank, world)
    eng.finish_all(comm, root)
    if rank == root:
        S = len(plan.samples()) if plan.sample_barcode else 1
        counts = [eng.render_wide_counts(s).decode("latin-1") for s in range(S)]
        merged = eng.render_wide_merged(list(reversed(range(S)))).decode("latin-1")
        with open(out, "w") as f:
            json.dump({"counts": counts, "merged": merged, "sorts": eng.wide_render_sorts()}, f)
    comm.barrier()
    comm.close()
    eng.close()


if __name__ == "__main__":
    main()
