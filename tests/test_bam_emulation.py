"""The BAM record framing of csrc/bc_bam.h -- header filter, successors, jump pointers, marks -- run on the host in
plain loops under AddressSanitizer and UndefinedBehaviorSanitizer (tests/bam/bam_host.cpp, a child process), over the
texts of bam_cases.py: it must find the writer's true record offsets, whatever decoys the text holds, and stay silent
under both sanitizers.  test_gpu_bam_frame.py asks the same of the kernels."""
import bam_cases


def test_the_host_framing_finds_the_writers_offsets(tmp_path):
    cases = bam_cases.cases()
    assert len(cases) >= 130
    got = bam_cases.run_host(cases, tmp_path)
    for c, (status, n_cand, end_pos, recs, _) in zip(cases, got):
        assert (status, end_pos, recs) == (c.status, c.end_pos, c.records), c.name
        assert n_cand >= len(recs), c.name
    by_name = {c.name: g for c, g in zip(cases, got)}
    for name in ("decoy_in_name", "decoy_in_z_aux", "decoy_in_b_array", "decoy_merges_into_the_chain"):  # the filter does let them in
        assert by_name[name][1] == len(by_name[name][3]) + 1, name
    assert by_name["decoy_chain_of_three"][1] == len(by_name["decoy_chain_of_three"][3]) + 3


def test_the_host_unpacking_is_what_samtools_fastq_writes(tmp_path):
    letters = bam_cases.NIBBLES
    recs = [bam_cases.Rec(seq=letters, qual=list(range(16))), bam_cases.Rec(flag=0x10, seq=letters + "A", qual=list(range(80, 97))),
            bam_cases.Rec(seq="ACGTT"), bam_cases.Rec(flag=0x10 | 0x40, seq="ACGTT"), bam_cases.Rec(seq=""),
            bam_cases.Rec(flag=0x10, seq="G", qual=[255]), bam_cases.Rec(seq="GA", qual=[0, 255]), bam_cases.Rec(flag=0x10, seq="AACCG", qual=[1, 2, 3, 4, 5])]
    case = bam_cases._whole("unpack", recs)
    (status, _, _, found, reads), = bam_cases.run_host([case], tmp_path, unpack=True)
    assert status == bam_cases.OK and found == case.records
    assert reads == [r.fastq() for r in recs]
    assert reads[1][0] == "T" + "".join(bam_cases.COMPLEMENT[c] for c in reversed(letters)) and reads[7] == ("CGGTT", "&%$#\"")
