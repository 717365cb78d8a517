"""One rank of a multi-process GPU test of the enrichment renderer (tests/test_gpu_enrich_render.py): counts its shard of
a seeded workload on device 0 (mp_rank.make_case), joins the job's exchange (bc_comm_create_host +
bc_engine_finish_all), and on the root writes the job's rows and the text of its Single / Double files
(bc_engine_render_enriched per sample, bc_engine_render_enriched_merged with the samples in descending order) as JSON.
    python tests/mp_rank_enrich_render.py <case> <rank> <world> <comm-dir> <n-total> <root> <out.json>"""
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
    if rank == root:
        eng.render_enriched(pkg.ENRICH_SINGLE, 0)  # this rank's share alone: its sums must not outlive the exchange
    comm = pkg.Comm.host(cdir, rank, world)
    counters, n_rows = eng.finish_all(comm, root)
    if rank == root:
        S = len(w.plan.samples()) if w.plan.sample_barcode else 1
        job = {"rows": eng.result_rows()}
        for name, kind in (("single", pkg.ENRICH_SINGLE), ("double", pkg.ENRICH_DOUBLE)):
            job[name] = [eng.render_enriched(kind, s).decode("latin-1") for s in range(S)]
            job[name + "_merged"] = eng.render_enriched_merged(kind, list(reversed(range(S)))).decode("latin-1")
        assert len(job["rows"]) == n_rows
        with open(out, "w") as f:
            json.dump(job, f)
    comm.barrier()
    comm.close()
    eng.close()


if __name__ == "__main__":
    main()
