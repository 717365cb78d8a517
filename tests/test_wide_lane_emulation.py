"""Wide keys on the lane-per-read kernel, on the host: csrc/bc_lane.h process_read<.., kWide> for plans lowered with
allow_wide, against (a) a byte-by-byte restatement of the key the wave-per-read kernel builds (tests/emu/wide_emu.cpp:
no bit planes, no shared layout helper) -- every matched read's key word for word, fingerprint included -- and (b) the
CPU oracle's outcome for every read.  The program runs under AddressSanitizer + UBSan, as a process of its own.
tests/test_gpu_wide_lane.py runs the same schemes through the kernel."""
import numpy as np
import pytest

import wide_emu_lib
import wide_lane_cases as wlc

UNSUPPORTED = 7


@pytest.mark.parametrize("name", sorted(wlc.SCHEMES))
def test_lane_key_equals_the_restated_key(name, tmp_path):
    c, pools, reads = wlc.pools_and_reads(name, 400, 5, p_sub=0.012, p_n=0.006)
    samples, counted = wlc.sets_of(c, pools)
    W, oc, key, ref_oc, ref_key = wide_emu_lib.run(c["scheme"], list(samples or []), counted, reads, tmp_path, tag=name)
    bits = sum(32 if ("samples_from" in c and k == c["samples_from"]) or k in c.get("counted_from", []) else 3 * ln
               for k, (_, ln) in enumerate(c["pools"]))
    assert W == 1 + (bits + 63) // 64 and 2 <= W <= 8
    o = wlc.oracle_of(c, pools)
    exp = np.array([wlc.twk.parity_code(o.process(r)) for r in reads], dtype=np.uint8)
    # (set membership -- the duplicates of a random-barcode plan -- is the insert's business: here a duplicate is matched)
    exp[exp == 4] = 0
    assert (oc == exp).all(), [(i, int(oc[i]), int(exp[i]), reads[i]) for i in np.nonzero(oc != exp)[0][:3]]
    assert (ref_oc == exp).all()
    m = oc == 0
    assert int(m.sum()) > 100
    assert (key[m] == ref_key[m]).all(), [(i, [hex(x) for x in key[i]], [hex(x) for x in ref_key[i]]) for i in np.nonzero((key != ref_key).any(1) & m)[0][:2]]
    assert (key[m, W:] == 0).all() and (key[m, 0] >> 63 == 0).all()
    assert any("N" in r for r in reads)  # (the third plane is in use)


def test_foreign_byte_in_a_raw_capture_or_the_random_barcode(tmp_path):
    c, pools, reads = wlc.pools_and_reads("raw_plus_random_28", 40, 9, p_sub=0.0, p_n=0.0, flank=(3, 3))
    reads[5] = reads[5][:3 + 6 + 10] + "x" + reads[5][3 + 6 + 11:]            # inside the 24-base raw capture
    reads[9] = reads[9][:3 + 6 + 24 + 4 + 27] + "R" + reads[9][3 + 6 + 24 + 4 + 28:]  # the random barcode's last base
    W, oc, key, ref_oc, ref_key = wide_emu_lib.run(c["scheme"], [], None, reads, tmp_path)
    exp = [UNSUPPORTED if i in (5, 9) else 0 for i in range(len(reads))]
    assert oc.tolist() == exp and ref_oc.tolist() == exp
    m = oc == 0
    assert (key[m] == ref_key[m]).all()


def test_all_n_leading_n_and_trailing_n_captures(tmp_path):
    c, pools, reads = wlc.pools_and_reads("raw_32", 12, 3, p_sub=0.0, p_n=0.0, flank=(2, 2))
    cap = slice(2 + 9, 2 + 9 + 32)
    put = lambda r, s: r[:cap.start] + s + r[cap.stop:]
    reads[0] = put(reads[0], "N" * 32)
    reads[1] = put(reads[1], "N" + reads[1][cap][1:])
    reads[2] = put(reads[2], reads[2][cap][:-1] + "N")
    W, oc, key, ref_oc, ref_key = wide_emu_lib.run(c["scheme"], [], None, reads, tmp_path)
    assert W == 3 and (oc == 0).all() and (ref_oc == 0).all()
    assert (key == ref_key).all()
    assert key[0, 1] == 0 and key[0, 2] == 0xFFFFFFFF  # planes 1 and 2 clear under 'N', the N plane full
    assert key[1, 2] & 1 and not key[1, 1] & 1 and not (key[1, 1] >> 32) & 1
    assert (key[2, 2] >> 31) & 1 and not (key[2, 1] >> 31) & 1 and not (key[2, 1] >> 63) & 1
