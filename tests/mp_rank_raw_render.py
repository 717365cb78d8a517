"""One rank of the multi-process raw-key render test (tests/test_gpu_raw_render.py): counts its shard of the seeded DEL
raw-key workload (raw_render_cases.del_raw_case) on device 0, joins the job's exchange (bc_comm_create_host +
bc_engine_finish_all), and on the root writes the text of the job's counts (bc_engine_render_raw_counts per sample,
bc_engine_render_raw_merged with the samples in descending order) as JSON.
    python tests/mp_rank_raw_render.py <rank> <world> <comm-dir> <n-total> <root> <out.json>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    rank, world, cdir, n_total, root, out = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]),
                                             int(sys.argv[5]), sys.argv[6])
    import torch
    import ngs_barcode_count_amd as pkg
    from ngs_barcode_count_amd import distributed as bcdist
    import raw_render_cases as rrc
    import readgen
    from test_gpu_parity import make_plan
    c = rrc.del_raw_case(n=n_total)
    plan = make_plan(c)
    first, count = bcdist.shard(n_total, rank, world)
    seq, _, lens = readgen.to_arrays(c["reads"][first:first + count], stride=100)
    eng = pkg.Engine(plan, device=0)
    if count:
        dseq = torch.from_numpy(seq.reshape(-1)).cuda()
        dlens = torch.from_numpy(lens.view("int16")).cuda()
        eng.submit_device(dseq.data_ptr(), None, count, 100, 100, dlens.data_ptr())
    comm = pkg.Comm.host(cdir, rank, world)
    eng.finish_all(comm, root)
    if rank == root:
        S = len(plan.samples())
        counts = [eng.render_raw_counts(s).decode("latin-1") for s in range(S)]
        merged = eng.render_raw_merged(list(reversed(range(S)))).decode("latin-1")
        with open(out, "w") as f:
            json.dump({"counts": counts, "merged": merged, "sorts": eng.raw_render_sorts()}, f)
    comm.barrier()
    comm.close()
    eng.close()


if __name__ == "__main__":
    main()
