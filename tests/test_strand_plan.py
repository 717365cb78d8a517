"""The strand setting of a plan (bc_plan_set_strand), on the host: default, round trip, refusal.  No GPU."""
import pytest

import cases
import strand_cases


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def test_default_is_forward():
    assert _pkg().Plan(cases.DEL_SCHEME).strand == "forward"


@pytest.mark.parametrize("strand", ["reverse", "both", "forward"])
def test_set_and_get_round_trip(strand):
    p = _pkg().Plan(cases.DEL_SCHEME)
    p.set_strand(strand)
    assert p.strand == strand
    p.set_strand("forward")
    assert p.strand == "forward"


@pytest.mark.parametrize("bad", ["", "Both", "rc", 2, None])
def test_invalid_name_is_refused(bad):
    p = _pkg().Plan(cases.DEL_SCHEME)
    p.set_strand("both")
    with pytest.raises(ValueError):
        p.set_strand(bad)
    assert p.strand == "both"


@pytest.mark.parametrize("bad", [-1, 3, 255])
def test_invalid_value_is_refused_by_the_library(bad):
    pkg = _pkg()
    p = pkg.Plan(cases.DEL_SCHEME)
    assert p._lib.bc_plan_set_strand(p._p, bad) == pkg._lib.BC_ERR_INVALID
    assert p.strand == "forward"
    assert [p._lib.bc_plan_set_strand(p._p, v) for v in (0, 1, 2)] == [0, 0, 0]


def test_python_rc_is_the_documented_table():
    """the helper the GPU tests compare against: IUPAC pairs in either case, everything else itself, an involution"""
    every = bytes(range(256))
    comp = strand_cases.rc_seq(every)[::-1]
    for a, b in zip("ATCGMKRYVBHD", "TAGCKMYRBVDH"):
        assert comp[ord(a)] == ord(b) and comp[ord(a.lower())] == ord(b.lower())
    moved = set(b"ATCGMKRYVBHDatcgmkryvbhd")
    assert all(comp[c] == c for c in range(256) if c not in moved)
    assert strand_cases.rc_seq(strand_cases.rc_seq(every)) == every
    assert strand_cases.rc("ACGTN", "abc") == ("NACGT", "cba")


def test_kernel_complement_table_on_the_host(tmp_path):
    """csrc/bc_strand_kernels.h strand_complement, compiled as host code under AddressSanitizer and UBSan (a stand-alone
    program): byte for byte the table of the Python rc()"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "complement_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(root, "tests", "strand", "complement_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert bytes.fromhex(out.stdout.strip()) == strand_cases.rc_seq(bytes(range(256)))[::-1]


@pytest.mark.parametrize("name", ["del_mismatch_quality", "crispr", "fmtn", "refs_with_n_and_ragged", "long_gaps"])
@pytest.mark.parametrize("ragged", [False, True])
def test_mixed_inputs_of_the_gpu_matrix_are_not_vacuous(name, ragged):
    """tests/test_gpu_strand.py's inputs, checked where no GPU is needed: see its assert_not_vacuous"""
    import test_gpu_strand
    test_gpu_strand.assert_not_vacuous(name, ragged)
