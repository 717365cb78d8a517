"""All four input paths of bc_fastq_count through ONE engine in ONE process, on one chunk size: plain text, BGZF inflated
on the device, ordinary gzip inflated on the device, gzip through zlib, plain again.  The ingest keeps its buffers from
call to call, so the set made for the plain file is upgraded for BGZF and then for gzip-device input rather than rebuilt;
every path must count the same reads."""
import os

import pytest

import bgzf
import cases
import gunzip_cases

pytestmark = pytest.mark.gpu

N_READS = 3000


def test_one_engine_counts_the_same_text_through_every_path(tmp_path, monkeypatch):
    import ngs_barcode_count_amd as pkg
    from test_gpu_parity import make_plan
    c = cases.build_case("del_mismatch_quality", n=N_READS)
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(c["reads"])).encode()
    plain, blocked, gz_dev, gz_zlib = (os.path.join(str(tmp_path), name) for name in
                                       ("a.fastq", "blocked.fastq.gz", "device.fastq.gz", "zlib.fastq.gz"))
    with open(plain, "wb") as f:
        f.write(text)
    bgzf.write(blocked, text, block_size=700)
    for path in (gz_dev, gz_zlib):
        with open(path, "wb") as f:
            f.write(gunzip_cases.gzip_member(text, 6))
    monkeypatch.setenv("BC_INGEST_CHUNK", "1048576")
    # (name, file, what the step sets; every other step runs with these three unset)
    device_env = {"BC_GZ_DEVICE": "all", "BC_GZ_SPAN_BYTES": "8192", "BC_GZ_PART_BYTES": "1024"}
    steps = [("plain", plain, {}), ("bgzf", blocked, {}), ("gzip_device", gz_dev, device_env), ("gzip_zlib", gz_zlib, {"BC_GZ_DEVICE": "1"}),
             ("plain_again", plain, {})]
    eng = pkg.Engine(make_plan(c), device=0)
    seen = {}
    try:
        before = (eng.counters(), eng.gz_blocks_inflated(), eng.gz_segments_inflated())
        for name, path, env in steps:
            for k in device_env:
                if k in env:
                    monkeypatch.setenv(k, env[k])
                else:
                    monkeypatch.delenv(k, raising=False)
            total = eng.count_fastq(path)
            after = (eng.counters(), eng.gz_blocks_inflated(), eng.gz_segments_inflated())
            # (reset_results gives a fresh table; the outcome counters go on, so a step's are the difference)
            seen[name] = dict(total=total, counters={k: after[0][k] - before[0][k] for k in after[0]}, rows=eng.result_rows(),
                              blocks=after[1] - before[1], segments=after[2] - before[2])
            print(name, total, seen[name]["counters"], "blocks", seen[name]["blocks"], "segments", seen[name]["segments"])
            before = after
            eng.reset_results()
    finally:
        eng.close()
    first = seen["plain"]
    assert first["counters"]["matched"] > 0 and first["rows"]
    for name, _, _ in steps:
        assert (seen[name]["counters"], seen[name]["rows"]) == (first["counters"], first["rows"]), name
    assert first["total"] == N_READS and seen["plain_again"]["total"] == N_READS
    assert seen["bgzf"]["total"] == seen["gzip_device"]["total"] == seen["gzip_zlib"]["total"]
    assert {n: seen[n]["blocks"] > 0 for n in seen} == {n: n == "bgzf" for n in seen}
    assert {n: seen[n]["segments"] > 0 for n in seen} == {n: n == "gzip_device" for n in seen}
    assert all(seen[n]["blocks"] == 0 for n in seen if n != "bgzf") and all(seen[n]["segments"] == 0 for n in seen if n != "gzip_device")
