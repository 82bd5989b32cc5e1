"""Every kernel path of the aligner against the oracle, and proof of which path ran.  GPU only.

device_align picks one of about a dozen kernel paths from the read lengths, k,
min_identity, the reduced cost matrix and the gap signs; sa_get_align_info reports
the choice.  Each row of tests/align_fixtures.py names a read set, settings, an
optional forced kernel / SA_P1_SEGS and the path it must take.  A row compares the
dispatch, every alignment field, the DUD / VALID / OVL_VALID flags and the .ovl
bytes with the oracle -- bit-exact, every element -- and asserts the align_info
fields it names, so a row cannot pass on another kernel than the one it is about.

Rows (ids): group16/32/64-* the lane-group kernel; lane16m / lane16x / lane24 /
lane32 -k2 / -k3 -i8 / -i16 the lane-per-pair kernels (masked, EXACT but not
packed, LW 24, LW 32; stored codes or path summaries; int8 or int16 costs); x2-*
the packed two-pairs-per-lane kernels with SA_P1_SEGS 0 / 1 / 2 / 5 / 8; gate652 /
gate653 either side of the packed-score gate; x2p1-* packed phase 1 followed by
the unpacked EXACT phase 2; quad-* the quadratic aligner; x2-strands both strands.
*-tie-* rows run tandem-repeat reads under HOXD70, +-1 costs with gaps -1 / -1 and
+-1 costs with gaps 0 / 0, where almost every cell ties (tests/test_align_fixtures.py
proves it on the oracle).
"""
import numpy as np
import pytest

import align_fixtures as F

pytestmark = pytest.mark.gpu

sao = pytest.importorskip("saoverlap")

ALIGN_CMP = ("start_i", "start_j", "end_i", "end_j", "correct", "error", "ahg", "bhg")


def compare(ov, r):
    """Dispatch, alignments, flags and .ovl bytes of a finished run against the oracle's."""
    lead, trail, _ = ov.dispatch()
    np.testing.assert_array_equal(lead, r.lead)
    np.testing.assert_array_equal(trail, r.trail)
    al = ov.alignments()
    assert len(al) == len(r.lead)
    for name in ALIGN_CMP:
        np.testing.assert_array_equal(al[:, sao.ALIGN_FIELDS.index(name)], r.align_field(name), err_msg=name)
    flags = al[:, sao.ALIGN_FIELDS.index("flags")]
    np.testing.assert_array_equal((flags & sao.FLAG_DUD) != 0, r.align_field("is_dud") != 0)
    np.testing.assert_array_equal((flags & sao.FLAG_VALID) != 0, r.align_field("valid") != 0)
    np.testing.assert_array_equal((flags & sao.FLAG_OVL_VALID) != 0,
                                  (r.align_field("ovl_valid") != 0) & (r.align_field("valid") != 0))
    assert ov.ovl() == r.ovl


@pytest.mark.parametrize("row_id", [r["id"] for r in F.ROWS if not r["strands"]])
def test_path(oracle_mod, monkeypatch, row_id):
    row = next(x for x in F.ROWS if x["id"] == row_id)
    if row["segs"] is not None:
        monkeypatch.setenv("SA_P1_SEGS", row["segs"])
    else:
        monkeypatch.delenv("SA_P1_SEGS", raising=False)
    r = F.oracle_run(oracle_mod, row)
    assert len(r.lead) >= 100
    with sao.Overlapper(aligner=sao.SA_ALIGNER_QUADRATIC if row["quadratic"] else sao.SA_ALIGNER_LINEAR,
                        align_kernel=row["align_kernel"], **row["st"]) as ov:
        ov.add_reads(F.row_reads(row))
        ov.build()
        with pytest.raises(sao.SAError) as e:
            ov.align_info()
        assert e.value.name == "SA_E_STATE"  # nothing aligned yet on this context
        ov.align()
        info = ov.align_info()
        assert {k: info[k] for k in row["expect"]} == row["expect"], info
        compare(ov, r)


def test_path_both_strands(oracle_mod, monkeypatch):
    """(f) both strands at a packed shape: the forward and the flipped block take the same
    path (sa_get_align_info fails if they ever differ), and both match the oracle."""
    import test_gpu_strands as S
    monkeypatch.delenv("SA_P1_SEGS", raising=False)
    row = next(x for x in F.ROWS if x["strands"])
    reads = F.row_reads(row)
    e = S.expected(oracle_mod, reads, True, **row["st"])
    assert len(e.r0.lead) >= 100 and e.n_lead_flipped + e.n_trail_flipped >= 100
    with S.gpu_run(reads, True, **row["st"]) as ov:
        info = ov.align_info()
        assert {k: info[k] for k in row["expect"]} == row["expect"], info
        S.compare(ov, e)
    # the flipped block alone is the 2N-read set's run: the same path when run by itself
    with sao.Overlapper(id_mode=sao.SA_IDS_WIDE, **row["st"]) as aug:
        aug.add_reads(reads + [S.rc(x) for x in reads])
        aug.build()
        aug.align()
        assert aug.align_info() == info


def test_align_info_on_a_sharded_context():
    with sao.Overlapper(shards=2, kmer_size=15, id_mode=sao.SA_IDS_WIDE) as ov:
        ov.add_reads(list(F.READS["x2"]()))
        ov.build()
        ov.align()
        with pytest.raises(sao.SAError) as e:
            ov.align_info()
        assert e.value.name == "SA_E_ARG"
