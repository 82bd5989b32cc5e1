"""Both-strand overlaps (SA_OPT_STRANDS = SA_STRANDS_BOTH) against the unchanged oracle.  GPU only.

The expected result is built from the oracle alone (include/sa_overlap.h, enum
sa_strands): the forward block is the oracle's run of the reads; the flipped block
is selected from its wide-id run D* of the 2N-read set "reads followed by their
reverse complements" -- the lead-flipped and trail-flipped classes, in D*'s order,
lead-flipped hangs transformed (ahg = -bhg', bhg = -ahg'), adj:I records.  Bar:
dispatch (ids, counts, strand codes), alignment tuples, flags and .ovl bytes are
bit-exact, every element.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

sao = pytest.importorskip("saoverlap")

ALIGN_CMP = ("start_i", "start_j", "end_i", "end_j", "correct", "error", "ahg", "bhg")
CLI = os.path.join(os.path.dirname(sao.LIB_PATH), "sa-overlap")
_RC = str.maketrans("ACGT", "TGCA")


def rc(s):
    """Reverse complement: A<->T, C<->G, every other byte itself."""
    return s[::-1].translate(_RC)


class Expected:
    """Forward block + flipped block of a both-strand run, from the oracle."""


def _counts(run, lead, trail, n_ids):
    """Collision counts of the (lead, trail) entries from the run's PairData."""
    key = run.pair_fst.astype(np.int64) * (n_ids + 1) + run.pair_snd
    order = np.argsort(key, kind="stable")
    want = lead.astype(np.int64) * (n_ids + 1) + trail
    pos = np.searchsorted(key[order], want)
    assert np.array_equal(key[order][pos], want)
    return run.pair_cnt[order][pos].astype(np.int32)


def expected(oracle_mod, reads, wide, **st):
    n = len(reads)
    r0 = oracle_mod.Run(reads=reads, settings=oracle_mod.default_settings(**st), wide=wide)
    r = oracle_mod.Run(reads=list(reads) + [rc(x) for x in reads], settings=oracle_mod.default_settings(**st),
                       wide=True)
    a, b = r.lead.astype(np.int64), r.trail.astype(np.int64)
    lf = (a > n) & (b <= n) & (a - n < b)      # lead flipped, strand code 2
    tf = (a <= n) & (b > n) & (a < b - n)      # trail flipped, strand code 1
    sel = np.flatnonzero(lf | tf)              # in D*'s order
    e = Expected()
    e.r0, e.r, e.n = r0, r, n
    e.n_lead_flipped, e.n_trail_flipped = int(lf.sum()), int(tf.sum())
    code = np.where(lf[sel], 2, 1).astype(np.uint8)
    f_lead = np.where(lf[sel], a[sel] - n, a[sel]).astype(np.int32)
    f_trail = np.where(tf[sel], b[sel] - n, b[sel]).astype(np.int32)
    e.lead = np.concatenate([r0.lead, f_lead])
    e.trail = np.concatenate([r0.trail, f_trail])
    e.count = np.concatenate([_counts(r0, r0.lead, r0.trail, n), _counts(r, r.lead[sel], r.trail[sel], 2 * n)])
    e.code = np.concatenate([np.zeros(len(r0.lead), dtype=np.uint8), code])
    fl = {name: r.align_field(name)[sel].copy() for name in ALIGN_CMP + ("is_dud", "valid", "ovl_valid")}
    ahg, bhg = fl["ahg"].copy(), fl["bhg"].copy()
    fl["ahg"] = np.where(code == 2, -bhg, ahg)
    fl["bhg"] = np.where(code == 2, -ahg, bhg)
    e.fields = {name: np.concatenate([r0.align_field(name), fl[name]]) for name in fl}
    keep = (fl["valid"] != 0) & (fl["ovl_valid"] != 0)
    e.flipped_records = (int((keep & (code == 2)).sum()), int((keep & (code == 1)).sum()))
    e.ovl = r0.ovl + b"".join(b"{OVL\nadj:I\nrds:%d,%d\nscr:0\nahg:%d\nbhg:%d\n}\n"
                              % (f_lead[i], f_trail[i], fl["ahg"][i], fl["bhg"][i]) for i in np.flatnonzero(keep))
    return e


def flipped_reads(n, length, genome, seed, mixed=None):
    """H.synth_reads with read i reverse-complemented where the seeded coin says so."""
    reads = H.synth_reads(n, length, genome, seed=seed, mixed=mixed)
    flip = np.random.default_rng(seed + 100).integers(0, 2, size=n)
    return [rc(x) if flip[i] else x for i, x in enumerate(reads)]


# (n, read length, genome, seed, mixed, settings, mutate, id modes: False strict / True wide)
CASES = [
    (64, 100, 600, 9, None, dict(kmer_size=12), False, (False, True)),
    (400, 120, 3000, 1, None, dict(kmer_size=12), False, (False, True)),
    (300, 200, 4000, 2, (80, 260), dict(kmer_size=15, min_collisions=3), False, (False, True)),
    (200, 90, 1200, 4, (40, 140), dict(kmer_size=16), False, (True,)),
    (300, 150, 2500, 3, None, dict(kmer_size=12, min_identity=0.95, min_collisions=5), True, (True,)),
    (40, 1200, 6000, 11, (1030, 1300), dict(kmer_size=15, max_collisions=2000, max_ignore=1300), False, (True,)),
]
CASE_IDS = [(c, w) for c in range(len(CASES)) for w in CASES[c][7]]


@functools.lru_cache(maxsize=None)
def case_reads(case):
    n, length, genome, seed, mixed, _, mut, _ = CASES[case]
    reads = flipped_reads(n, length, genome, seed, mixed)
    if mut:
        reads = H.mutate(reads, np.random.default_rng(5), 2)
    return tuple(reads)


_expected_cache = {}


def case_expected(oracle_mod, case, wide):
    """The oracle's answer for a case, computed once and shared (never modified)."""
    if (case, wide) not in _expected_cache:
        _expected_cache[(case, wide)] = expected(oracle_mod, list(case_reads(case)), wide, **CASES[case][5])
    return _expected_cache[(case, wide)]


def gpu_run(reads, wide, strands=sao.STRANDS_BOTH, **kw):
    ov = sao.Overlapper(id_mode=sao.SA_IDS_WIDE if wide else sao.SA_IDS_STRICT, strands=strands, **kw)
    ov.add_reads(reads)
    ov.build()
    ov.align()
    return ov


def compare(ov, e):
    assert e.n_lead_flipped > 0 and e.n_trail_flipped > 0
    lead, trail, count = ov.dispatch()
    np.testing.assert_array_equal(lead, e.lead)
    np.testing.assert_array_equal(trail, e.trail)
    np.testing.assert_array_equal(count, e.count)
    np.testing.assert_array_equal(ov.dispatch_strands(), e.code)
    al = ov.alignments()
    assert len(al) == len(e.lead)
    for name in ALIGN_CMP:
        np.testing.assert_array_equal(al[:, sao.ALIGN_FIELDS.index(name)], e.fields[name], err_msg=name)
    flags = al[:, sao.ALIGN_FIELDS.index("flags")]
    np.testing.assert_array_equal((flags & sao.FLAG_DUD) != 0, e.fields["is_dud"] != 0)
    np.testing.assert_array_equal((flags & sao.FLAG_VALID) != 0, e.fields["valid"] != 0)
    np.testing.assert_array_equal((flags & sao.FLAG_OVL_VALID) != 0,
                                  (e.fields["ovl_valid"] != 0) & (e.fields["valid"] != 0))
    np.testing.assert_array_equal((flags & sao.FLAG_FLIP_TRAIL) != 0, e.code == 1)
    np.testing.assert_array_equal((flags & sao.FLAG_FLIP_LEAD) != 0, e.code == 2)
    # flipped entries carry their original ids
    fl = e.code != 0
    np.testing.assert_array_equal(al[fl, sao.ALIGN_FIELDS.index("lead")], e.lead[fl])
    np.testing.assert_array_equal(al[fl, sao.ALIGN_FIELDS.index("trail")], e.trail[fl])
    assert ov.ovl() == e.ovl
    st = ov.stats()
    assert st["dispatched"] == st["aligned"] == len(e.lead)
    assert st["ovl_records"] == e.ovl.count(b"{OVL")


@pytest.mark.parametrize("case,wide", CASE_IDS)
def test_both_strands_match_oracle(oracle_mod, case, wide):
    """Forward block (strict Trove order or wide order) then the flipped block of D*."""
    e = case_expected(oracle_mod, case, wide)
    if case == len(CASES) - 1:
        # reads above 1,024 bases: the shape must pass with the option off first
        with gpu_run(list(case_reads(case)), wide, strands=sao.STRANDS_FORWARD, **CASES[case][5]) as fwd:
            assert fwd.ovl() == e.r0.ovl
    with gpu_run(list(case_reads(case)), wide, **CASES[case][5]) as ov:
        compare(ov, e)


def test_non_acgt_passes_through(oracle_mod):
    """A read with N bases that no dispatched alignment touches: result as the oracle's."""
    reads = list(case_reads(0))
    rng = np.random.default_rng(77)
    odd = list("".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=100)))
    odd[3] = "N"
    odd[60] = odd[61] = "N"
    reads.insert(30, "".join(odd))
    st = CASES[0][5]
    e = expected(oracle_mod, reads, True, **st)
    with gpu_run(reads, True, **st) as ov:
        compare(ov, e)


def test_non_acgt_error(oracle_mod):
    """An N inside aligned regions fails the call as it fails the oracle (-3)."""
    reads = list(case_reads(0))
    reads[0] = reads[0][:50] + "N" + reads[0][51:]
    st = CASES[0][5]
    for rs in (reads, reads + [rc(x) for x in reads]):
        with pytest.raises(oracle_mod.OracleError) as oe:
            oracle_mod.Run(reads=rs, settings=oracle_mod.default_settings(**st), wide=True)
        assert oe.value.rc == -3
    ov = sao.Overlapper(id_mode=sao.SA_IDS_WIDE, strands=sao.STRANDS_BOTH, **st)
    ov.add_reads(reads)
    ov.build()
    with pytest.raises(sao.SAError) as ge:
        ov.align()
    assert ge.value.name == "SA_E_NON_ACGT"
    ov.close()


def test_off_means_off(oracle_mod):
    """Never set, or set to SA_STRANDS_FORWARD: a plain run, all strand codes 0."""
    reads = list(case_reads(1))
    st = CASES[1][5]
    e = case_expected(oracle_mod, 1, True)
    res = []
    for explicit in (False, True):
        ov = sao.Overlapper(id_mode=sao.SA_IDS_WIDE, **st)
        if explicit:
            ov.set_strands(sao.STRANDS_FORWARD)
        ov.add_reads(reads)
        ov.build()
        ov.align()
        res.append((ov.dispatch(), ov.alignments(), ov.ovl(), ov.stats()))
        codes = ov.dispatch_strands()
        assert len(codes) == len(e.r0.lead) and not codes.any()
        ov.close()
    for x, y in zip(res[0][0], res[1][0]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(res[0][0][0], e.r0.lead)
    np.testing.assert_array_equal(res[0][0][1], e.r0.trail)
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2] == e.r0.ovl
    assert res[0][3] == res[1][3]
    flags = res[0][1][:, sao.ALIGN_FIELDS.index("flags")]
    assert not (flags & (sao.FLAG_FLIP_TRAIL | sao.FLAG_FLIP_LEAD)).any()


def test_stats_determinism_afg(oracle_mod, tmp_path):
    reads = list(case_reads(1))
    st = CASES[1][5]
    e = case_expected(oracle_mod, 1, True)
    with gpu_run(reads, True, strands=sao.STRANDS_FORWARD, **st) as fwd:
        fwd_kmers = fwd.stats()["kmers"]
    with gpu_run(reads, True, **st) as ov:
        s1 = ov.stats()
        assert s1["kmers"] == 2 * fwd_kmers
        assert s1["pairs"] == len(e.r.pair_fst)
        d1, c1, o1 = ov.dispatch(), ov.dispatch_strands(), ov.ovl()
        afg = str(tmp_path / "both.afg")
        ov.write_afg(afg)
        blob = open(afg, "rb").read()
        assert blob.endswith(o1) and blob.count(b"{OVL") == o1.count(b"{OVL")
        ov.build()   # a second build on the same context
        ov.align()
        for x, y in zip(d1, ov.dispatch()):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(c1, ov.dispatch_strands())
        assert ov.ovl() == o1 == e.ovl
        # switching the option off again gives the plain run
        ov.set_strands(sao.STRANDS_FORWARD)
        ov.build()
        ov.align()
        assert ov.ovl() == e.r0.ovl and not ov.dispatch_strands().any()


def test_device_only_calls_then_getters(oracle_mod):
    """sa_device_build / sa_device_align (no readback), then the getters fetch both blocks."""
    e = case_expected(oracle_mod, 2, True)
    ov = sao.Overlapper(id_mode=sao.SA_IDS_WIDE, strands=sao.STRANDS_BOTH, timing=True, **CASES[2][5])
    ov.add_reads(list(case_reads(2)))
    ov.device_build()
    ov.device_align()
    ov.sync()
    compare(ov, e)
    t = ov.stage_times()
    assert t["pack"][1] >= 1 and t["order"][1] >= 2   # revcomp under pack, the strand filter under order
    ov.close()


def test_refusals():
    def refused(fn):
        with pytest.raises(sao.SAError) as err:
            fn()
        assert err.value.name == "SA_E_ARG"

    with sao.Overlapper(shards=2, id_mode=sao.SA_IDS_WIDE) as ov:
        refused(lambda: ov.set_strands(sao.STRANDS_BOTH))
    with sao.Overlapper(aligner=sao.SA_ALIGNER_QUADRATIC) as ov:
        refused(lambda: ov.set_strands(sao.STRANDS_BOTH))
    with sao.Overlapper(keep_pairs=True) as ov:
        refused(lambda: ov.set_strands(sao.STRANDS_BOTH))
    # ... and whichever option is set second
    with sao.Overlapper(strands=sao.STRANDS_BOTH) as ov:
        refused(lambda: ov.set_aligner(sao.SA_ALIGNER_QUADRATIC))
        refused(lambda: ov._chk(sao.lib().sa_set_option(ov.h, sao.SA_OPT_KEEP_PAIRS, 1)))
        refused(lambda: ov.set_strands(7))


def test_cli_both_strands(oracle_mod, tmp_path):
    reads = list(case_reads(0))
    fasta, out = str(tmp_path / "reads.seq"), str(tmp_path / "out.ovl")
    open(fasta, "wb").write(H.reads_fasta_bytes(reads))
    r = subprocess.run([CLI, "-i", fasta, "-o", out, "-k", "12", "--both-strands"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == case_expected(oracle_mod, 0, False).ovl   # (AUTO ids: strict here)
    r = subprocess.run([CLI, "-i", fasta, "-o", out, "-k", "12", "--both-strands", "--shards", "2"],
                       capture_output=True)
    assert r.returncode == 1
    r = subprocess.run([CLI, "-i", fasta, "-o", out, "-k", "12", "--forward-strand"], capture_output=True)
    assert r.returncode == 0 and open(out, "rb").read() == case_expected(oracle_mod, 0, False).r0.ovl
