"""Alignment error codes: SA_E_SHORT_READ and SA_E_DEGENERATE on every kernel that sets them.  GPU only.

The reference crashes (StringIndexOutOfBounds) on a trail shorter than its lead's
band and on a phase-1 matrix with no positive cell; the oracle reports both as
ORC_E_INDEX and the device as SA_E_SHORT_READ / SA_E_DEGENERATE.  Each fixture
below holds exactly one kind of failing pair: the same reads with the failing
read swapped for an ordinary one align without error (asserted on the oracle),
so the code the device returns is that pair's.  Mixed sets are not tested: with
several failing pairs the device reports whichever arrives first
(include/sa_overlap.h, enum sa_status).

After a failed alignment the getters give SA_E_STATE and sa_get_align_info still
names the path that was attempted.  A context has no call that takes reads back,
so recovery is shown in two steps: the same context aligns the same reads with
the quadratic aligner (which has neither error) to the oracle's result, and a
context of the same settings aligns the repaired read set to the oracle's.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sao = pytest.importorskip("saoverlap")

from test_gpu_align_paths import compare  # noqa: E402

HOXD70 = [91, -114, -31, -123, -114, 100, -125, -31, -31, -125, 100, -114, -123, -31, -114, 91]
HOXD_I16 = [1000] + HOXD70[1:15] + [910]
# (kernel option, expected align_info kernel)
KERNELS = {"auto": (sao.ALIGN_AUTO, None), "group": (sao.ALIGN_GROUP, 1), "lane": (sao.ALIGN_LANE, 2),
           "lane_summary": (sao.ALIGN_LANE_SUMMARY, 3)}


def genome(seed, n, alphabet="ACGT"):
    rng = np.random.default_rng(seed)
    return "".join(alphabet[x] for x in rng.integers(0, len(alphabet), n))


@functools.lru_cache(maxsize=None)
def short_trail_set(with_n=False):
    """1,000 bp leads (band 20) tiled over a genome, and one 16 bp trail cut from the end
    of the last lead, a stretch no other lead covers: it meets that lead only, as a trail
    shorter than the band.  with_n: the 16 bp read also holds an N (two errors in one pair;
    the reference meets the length first)."""
    g = genome(51, 2200)
    leads = [g[s:s + 1000] for s in range(0, 1201, 100)]
    short = leads[-1][978:994]
    if with_n:
        short = short[:14] + "N" + short[15:]
    good = g[600:1600]
    return tuple(leads + [short]), tuple(leads + [good])


SHORT_ST = dict(kmer_size=12, min_collisions=1, max_collisions=10 ** 7, max_ignore=2000)


@functools.lru_cache(maxsize=None)
def degenerate_set(length):
    """G/T-only leads of `length` bp and one trail that opens with 40 A (its first `width`
    bases score below zero against every lead base, so phase 1 has no positive cell) and
    carries the end of the first lead in its middle, which is what dispatches the pair."""
    g = genome(52, 3 * length, "GT")
    leads = [g[s:s + length] for s in range(0, 2 * length + 1, length // 8)]
    mid = leads[0][-45:-5]
    trail = "A" * 40 + mid + "A" * 40
    good = g[length // 16:length // 16 + length]
    return tuple(leads + [trail]), tuple(leads + [good])


def st_key(st):
    return tuple(sorted((k, tuple(v) if k == "cost" else v) for k, v in st.items()))


_oracle = {}


def oracle_of(oracle_mod, reads, quadratic=False, **st):
    """Oracle runs are shared between the tests (never modified); a failing run is kept as
    its OracleError."""
    key = (reads, quadratic, st_key(st))
    if key not in _oracle:
        try:
            _oracle[key] = oracle_mod.Run(reads=list(reads), settings=oracle_mod.default_settings(**st),
                                          quadratic=quadratic)
        except oracle_mod.OracleError as e:
            _oracle[key] = e
    return _oracle[key]


def expect_failure(oracle_mod, bad, good, name, kernel, info=None, **st):
    """The oracle fails on `bad` with ORC_E_INDEX and not on `good`.  The device fails on
    `bad` with `name`, keeps no records and still reports the attempted path; the same
    context then aligns `bad` with the quadratic aligner (which has neither error) to the
    oracle's result; and a context of the same settings aligns `good` to the oracle's.
    (A context has no call that takes reads back, so the repaired set needs its own.)"""
    e = oracle_of(oracle_mod, bad, **st)
    assert isinstance(e, oracle_mod.OracleError) and e.rc == oracle_mod.ORC_E_INDEX
    r = oracle_of(oracle_mod, good, **st)
    assert not isinstance(r, Exception) and len(r.lead) > 20
    rq = oracle_of(oracle_mod, bad, quadratic=True, **st)
    opt, want_kernel = KERNELS[kernel]
    with sao.Overlapper(align_kernel=opt, **st) as ov:
        ov.add_reads(list(bad))
        ov.build()
        for align in (ov.align, ov.device_align):
            with pytest.raises(sao.SAError) as err:
                align()
            assert err.value.name == name
            for getter in (ov.alignments, ov.ovl, ov.write_ovl):
                with pytest.raises(sao.SAError) as err:
                    getter()
                assert err.value.name == "SA_E_STATE"
            got = ov.align_info()
            if want_kernel is not None:
                assert got["kernel"] == want_kernel
            for k, v in (info or {}).items():
                assert got[k] == v, got
        ov.set_aligner(sao.SA_ALIGNER_QUADRATIC)
        if isinstance(rq, Exception):  # (the trail with an N: the full matrix reaches it)
            assert rq.rc == oracle_mod.ORC_E_MATCH
            with pytest.raises(sao.SAError) as err:
                ov.align()
            assert err.value.name == "SA_E_NON_ACGT"
        else:
            ov.align()
            assert ov.align_info()["kernel"] == 4
            compare(ov, rq)
    with sao.Overlapper(align_kernel=opt, **st) as ov:
        ov.add_reads(list(good))
        ov.build()
        ov.align()
        compare(ov, r)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_short_trail(oracle_mod, kernel):
    """SA_E_SHORT_READ: a 16 bp trail against a 1,000 bp lead whose band is 20, on the
    lane-group kernel, both lane-per-pair kernels and the automatic choice (LW = 24).  The
    EXACT and packed kernels cannot meet it: their bands are 15 = k, and a dispatched
    trail holds at least one k-mer, so it is never shorter than the band."""
    bad, good = short_trail_set()
    expect_failure(oracle_mod, bad, good, "SA_E_SHORT_READ", kernel,
                   info=dict(width=32 if kernel == "group" else 24, exact=0), **SHORT_ST)


@pytest.mark.parametrize("kernel", ["group", "lane"])
def test_short_trail_with_an_n_is_short_first(oracle_mod, kernel):
    """One pair with two errors: the 16 bp trail also holds an N.  The reference indexes
    past the trail before it looks the N up, so the answer is ORC_E_INDEX / SA_E_SHORT_READ."""
    bad, good = short_trail_set(with_n=True)
    assert "N" in bad[-1]
    expect_failure(oracle_mod, bad, good, "SA_E_SHORT_READ", kernel, **SHORT_ST)


DEGEN_ST = dict(min_collisions=1, max_collisions=10 ** 7, max_ignore=2000)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_degenerate_phase1(oracle_mod, kernel):
    """SA_E_DEGENERATE on the masked kernels: 300 bp G/T-only leads at k = 12 (band 12)."""
    bad, good = degenerate_set(300)
    expect_failure(oracle_mod, bad, good, "SA_E_DEGENERATE", kernel,
                   info=dict(width=16, exact=0), kmer_size=12, **DEGEN_ST)


@pytest.mark.parametrize("case", ["packed", "packed_segs0", "exact_int16", "exact_int16_summary"])
def test_degenerate_phase1_exact_kernels(oracle_mod, monkeypatch, case):
    """SA_E_DEGENERATE at k = 15 on 500 bp leads (every band 15): the packed phase 1 in row
    segments and as one segment, and the unpacked EXACT phase 1 (int16 costs)."""
    bad, good = degenerate_set(500)
    monkeypatch.delenv("SA_P1_SEGS", raising=False)
    if case == "packed_segs0":
        monkeypatch.setenv("SA_P1_SEGS", "0")
    if case.startswith("packed"):
        expect_failure(oracle_mod, bad, good, "SA_E_DEGENERATE", "auto",
                       info=dict(kernel=2, exact=1, p1_x2=1, nseg=0 if case == "packed_segs0" else 8),
                       kmer_size=15, **DEGEN_ST)
    else:
        expect_failure(oracle_mod, bad, good, "SA_E_DEGENERATE", "lane_summary" if case.endswith("summary") else "lane",
                       info=dict(exact=1, p1_x2=0, cost_bits=16), kmer_size=15, cost=tuple(HOXD_I16), **DEGEN_ST)


def test_quadratic_aligner_has_no_degenerate_error(oracle_mod):
    """The full-matrix aligner finds the shared middle wherever it lies: the oracle reports
    no error on the degenerate set, and the device agrees field for field."""
    bad, _ = degenerate_set(300)
    st = dict(kmer_size=12, **DEGEN_ST)
    r = oracle_of(oracle_mod, bad, quadratic=True, **st)
    assert not isinstance(r, Exception) and len(r.lead) > 20
    with sao.Overlapper(aligner=sao.SA_ALIGNER_QUADRATIC, **st) as ov:
        ov.add_reads(list(bad))
        ov.build()
        ov.align()
        assert ov.align_info()["kernel"] == 4
        compare(ov, r)


def test_no_candidates_at_a_packed_shape():
    """No dispatched pair at a shape that selects the packed kernels: an empty alignment,
    not a division by the zero wave count."""
    reads = [genome(60 + i, 480) for i in range(4)]
    with sao.Overlapper(kmer_size=15) as ov:
        ov.add_reads(reads)
        ov.build()
        assert len(ov.dispatch()[0]) == 0
        ov.align()
        assert len(ov.alignments()) == 0 and ov.ovl() == b""
        assert ov.align_info()["p1_x2"] == 1
