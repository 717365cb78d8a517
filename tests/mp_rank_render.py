"""One rank of a multi-process GPU render test (tests/test_gpu_render.py): counts its shard of a seeded workload on
device 0 (mp_rank.make_case), joins the job's exchange (bc_comm_create_host + bc_engine_finish_all), and on the root
writes the job's rows and the text of its counts (bc_engine_render_counts per sample, bc_engine_render_merged with the
samples in descending order) as JSON.
    python tests/mp_rank_render.py <case> <rank> <world> <comm-dir> <n-total> <root> <out.json>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    case, rank, world, cdir, n_total, root, out = (sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4],
                                                   int(sys.argv[5]), int(sys.argv[6]), sys.argv[7])
    import torch
    import ngs_barcode_count_amd as pkg
    from ngs_barcode_count_amd import distributed as bcdist
    from mp_rank import make_case
    w = make_case(case)
    first, count = bcdist.shard(n_total, rank, world)
    eng = pkg.Engine(w.plan, device=0)
    R = w.read_len
    if count:
        dseq = torch.empty(count * R, dtype=torch.uint8, device="cuda")
        dqual = torch.empty(count * R, dtype=torch.uint8, device="cuda")
        w.synth.generate_device(0, None, first, count, dseq.data_ptr(), dqual.data_ptr())
        torch.cuda.synchronize()
        eng.submit_device(dseq.data_ptr(), dqual.data_ptr() if w.min_quality > 0 else None, count, R, R)
    comm = pkg.Comm.host(cdir, rank, world)
    counters, n_rows = eng.finish_all(comm, root)
    if rank == root:
        S = len(w.plan.samples()) if w.plan.sample_barcode else 1
        counts = [eng.render_counts(s).decode("latin-1") for s in range(S)]
        merged = eng.render_merged(list(reversed(range(S)))).decode("latin-1")
        rows = eng.result_rows()
        assert len(rows) == n_rows
        with open(out, "w") as f:
            json.dump({"rows": rows, "counts": counts, "merged": merged}, f)
    comm.barrier()
    comm.close()
    eng.close()


if __name__ == "__main__":
    main()
