"""CPU checks of the both-strand expectation built in test_gpu_strands.py: the oracle's
run of the 2N-read set "reads followed by their reverse complements" defines the new
mode without being changed -- its forward x forward part is today's wide dispatch, the
flipped classes are non-empty and mirror-symmetric, lead-flipped entries come first."""
import numpy as np
import pytest

import test_gpu_strands as S


@pytest.mark.parametrize("case", range(len(S.CASES)))
def test_expected_sets(oracle_mod, case):
    e = S.case_expected(oracle_mod, case, True)
    n, r = e.n, e.r
    print("case %d: lead-flipped %d trail-flipped %d .ovl records (lead / trail) %s duds in D* %d"
          % (case, e.n_lead_flipped, e.n_trail_flipped, e.flipped_records, int((r.align_field("is_dud") != 0).sum())))
    assert e.n_lead_flipped > 0 and e.n_trail_flipped > 0
    a, b = r.lead.astype(np.int64), r.trail.astype(np.int64)
    # the forward x forward part of D* is the wide dispatch of the reads alone
    ff = (a <= n) & (b <= n)
    r0 = e.r0
    np.testing.assert_array_equal(a[ff], r0.lead)
    np.testing.assert_array_equal(b[ff], r0.trail)
    for name in S.ALIGN_CMP:
        np.testing.assert_array_equal(r.align_field(name)[ff], r0.align_field(name), err_msg=name)
    # every kept flipped pair has its mirror duplicate in D* (dropped): (a, b) <-> (b', a')
    # with x' the other strand of x
    other = lambda x: np.where(x > n, x - n, x + n)
    have = set(zip(a.tolist(), b.tolist()))
    code = e.code[e.code != 0]
    sel = np.flatnonzero(((a > n) & (b <= n) & (a - n < b)) | ((a <= n) & (b > n) & (a < b - n)))
    for x, y in zip(other(b[sel]).tolist(), other(a[sel]).tolist()):
        assert (x, y) in have
    # lead descending: every lead-flipped entry precedes every trail-flipped one
    assert (np.diff(code.astype(np.int32)) <= 0).all()
    assert e.ovl.startswith(r0.ovl) and e.ovl.count(b"adj:I") == sum(e.flipped_records)
    assert sum(e.flipped_records) > 0
