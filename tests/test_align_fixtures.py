"""The aligner fixtures do what they claim -- checked on the CPU oracle alone.

tests/test_gpu_align_paths.py compares every kernel path with the oracle on the
read sets of tests/align_fixtures.py.  That only closes a gap if the inputs reach
the places where kernels go wrong: cells that tie for the maximum (the
reference's argmax keeps the first in row-major order), backtrack steps where
M / X / Y tie (it prefers M over X over Y), scores next to the packed 16-bit
limit, and the kernel path each row names.  These tests assert those conditions
on the inputs, through the oracle's diagnostic entry orc_align_pair_diag, and
never touch a kernel.
"""
import numpy as np
import pytest

import align_fixtures as F
import literal

LINEAR_ROWS = [r for r in F.ROWS if not r["quadratic"] and not r["strands"]]
_diag_cache = {}


def diag(oracle_mod, r):
    """Per dispatched pair of a row: the oracle's tie diagnostics (one dict of columns),
    computed once per distinct oracle run."""
    run = F.oracle_run(oracle_mod, r)
    if id(run) not in _diag_cache:
        al, dg = oracle_mod.align_batch_diag(F.row_reads(r), run.lead, run.trail,
                                             oracle_mod.default_settings(**r["st"]))
        # the diagnostic entry computes the alignments orc_run does
        np.testing.assert_array_equal(al, run.aligns)
        _diag_cache[id(run)] = {n: dg[:, i] for i, n in enumerate(oracle_mod.DIAG_FIELDS)}
    return _diag_cache[id(run)]


def tie_counts(d):
    """(pairs whose phase-1 maximum is attained by several cells, pairs with at least one tied
    backtrack step, tied steps in all)."""
    steps = d["p1_tied"] + d["p2_tied"]
    return int((d["p1_cells"] > 1).sum()), int((steps > 0).sum()), int(steps.sum())


def literal_settings(st):
    s = dict(F.DEFAULTS, cost=F.HOXD70)
    s.update(st)
    c = s["cost"]
    return literal.AlignSettings(k=s["kmer_size"], gap_open=s["gap_open"], gap_extend=s["gap_extend"],
                                 min_identity=s["min_identity"], cost=[list(c[4 * a:4 * a + 4]) for a in range(4)])


@pytest.mark.parametrize("row_id", ["group16-tie-hoxd", "x2-tie-pm1g1", "x2-tie-pm1g0", "lane24-k2-tie-pm1g0",
                                    "lane16m-k2-i8"])
def test_diag_agrees_with_instrumented_literal(oracle_mod, row_id):
    """orc_align_pair_diag against literal.fast_dovetail(diag=...) on 4 pairs of each of 5
    fixtures (20 pairs): the six diagnostic fields and the alignment; and its alignment
    is orc_align_pair's, field for field."""
    r = next(x for x in F.ROWS if x["id"] == row_id)
    run = F.oracle_run(oracle_mod, r)
    reads = F.row_reads(r)
    st = oracle_mod.default_settings(**r["st"])
    ls = literal_settings(r["st"])
    live = np.flatnonzero(run.align_field("is_dud") == 0)
    picks = list(live[:: max(1, len(live) // 3)][:3]) + list(np.flatnonzero(run.align_field("is_dud") != 0)[:1])
    if len(picks) < 4:
        picks.append(int(live[1]))
    for p in picks:
        a, b = int(run.lead[p]), int(run.trail[p])
        al, dg = oracle_mod.align_pair_diag(reads[a - 1], reads[b - 1], a, b, settings=st)
        assert al == oracle_mod.align_pair(reads[a - 1], reads[b - 1], a, b, settings=st)
        want = {}
        la = literal.fast_dovetail(a, reads[a - 1], b, reads[b - 1], ls, want)
        assert dg == want, (row_id, a, b)
        if la is literal.DUD:
            assert al["is_dud"] == 1 and dg["p2_max"] == dg["p2_cells"] == dg["p2_tied"] == 0
        else:
            assert (al["start_i"], al["start_j"]) == la.start and (al["end_i"], al["end_j"]) == la.end
            assert (al["correct"], al["error"]) == (la.correct, la.error)


def test_tie_heavy_fixtures_tie(oracle_mod):
    """Every tie-heavy fixture (tandem reads x cost setting x band) has >= 50 dispatched
    pairs whose phase-1 maximum several cells attain and >= 50 pairs with a tied backtrack step."""
    seen = set()
    for r in LINEAR_ROWS:
        if not r["tie"] or id(F.oracle_run(oracle_mod, r)) in seen:
            continue
        seen.add(id(F.oracle_run(oracle_mod, r)))
        multi, tied, steps = tie_counts(diag(oracle_mod, r))
        n = len(F.oracle_run(oracle_mod, r).lead)
        print("%-24s %5d pairs: %5d with a multiply-attained phase-1 maximum, %5d with a tied backtrack step "
              "(%d steps)" % (r["id"], n, multi, tied, steps))
        assert multi >= 50, r["id"]
        assert tied >= 50, r["id"]
    assert len(seen) >= 12


def test_random_hoxd70_sets_hardly_tie(oracle_mod):
    """The gap being closed: on the random-genome HOXD70 sets the aligner tests used so far
    (test_gpu_hoxd.py's three read sets) a maximum attained by two cells is a rarity -- under
    1 % of the pairs, against ~99 % on the tandem reads -- so the first-in-row-major argmax
    rule was hardly exercised.  Tied backtrack steps are a different matter, and the counts
    are printed, not bounded: these reads carry indels, and an indel inside a run of equal
    bases ties (gap-then-match scores what match-then-gap does), so ~40 % of their pairs
    already hold a tied step or two.  What the tandem reads add there is the +-1 / gap 0
    setting, with several tied steps per pair and ties of all three of M / X / Y."""
    for rid in ("lane16m-k2-i8", "x2-rand", "x2-segs0"):
        r = next(x for x in F.ROWS if x["id"] == rid)
        assert r["reads"] in ("short", "x2", "x2b") and tuple(r["st"].get("cost", F.HOXD70)) == F.HOXD70
        d = diag(oracle_mod, r)
        multi, tied, steps = tie_counts(d)
        n = len(d["p1_cells"])
        print("%-24s %5d pairs: %5d with a multiply-attained phase-1 maximum, %5d with a tied backtrack step "
              "(%d steps, %.2f per pair)" % (rid, n, multi, tied, steps, steps / n))
        assert multi * 100 < n, rid


def test_gate_fixture_reaches_the_16_bit_limit(oracle_mod):
    """(c): the 652 bp C/G set holds a pair whose phase-2 maximum is 100 x 652 = 65,200, within
    336 of the packed kernels' limit; the 653 bp set goes to 65,300, past what they accept."""
    for rid, top in (("gate652", 65200), ("gate653", 65300)):
        d = diag(oracle_mod, next(x for x in F.ROWS if x["id"] == rid))
        print(rid, "largest phase-2 maximum", int(d["p2_max"].max()), "pairs >= 65,000:",
              int((d["p2_max"] >= 65000).sum()))
        assert d["p2_max"].max() == top >= 65000


@pytest.mark.parametrize("row_id", F.ROW_IDS)
def test_expected_path_follows_from_the_fixture(oracle_mod, row_id):
    """The align_info a row expects is what the selection rule gives for its read lengths and
    settings, and the row dispatches at least 100 pairs."""
    r = next(x for x in F.ROWS if x["id"] == row_id)
    run = F.oracle_run(oracle_mod, r)
    assert len(run.lead) >= 100
    got = F.select_path([len(x) for x in F.row_reads(r)], r["st"], r["quadratic"], r["align_kernel"], r["segs"],
                        len(run.lead))
    assert {k: got[k] for k in r["expect"]} == r["expect"]


def test_table_covers_every_path(oracle_mod):
    """Every kernel path of device_align appears in the table, with duds and invalid overlaps."""
    seen = set()
    for r in F.ROWS:
        e = F.select_path([len(x) for x in F.row_reads(r)], r["st"], r["quadratic"], r["align_kernel"], r["segs"],
                          len(F.oracle_run(oracle_mod, r).lead))
        seen.add((e["kernel"], e["width"], e["exact"], e["p1_x2"], e["p2_x2"], e["cost_bits"]))
        if e["p1_x2"]:
            seen.add(("nseg", e["p2_x2"], e["nseg"]))
    want = {(1, g, 0, 0, 0, 8) for g in (16, 32, 64)}
    want |= {(kn, lw, 0, 0, 0, b) for kn in (2, 3) for lw in (16, 24, 32) for b in (8, 16)}
    want |= {(kn, 16, 1, 0, 0, b) for kn in (2, 3) for b in (8, 16)}         # EXACT, not packed
    want |= {(2, 16, 1, 1, 1, 8), (2, 16, 1, 1, 0, 8), (3, 16, 1, 1, 0, 8)}  # packed p1 + p2tbx2 / p2tb / summaries
    want |= {(4, 0, 0, 0, 0, 8)}
    want |= {("nseg", 1, n) for n in (0, 1, 2, 5, 8)} | {("nseg", 0, 0), ("nseg", 0, 8)}
    assert want <= seen, want - seen
    duds = sum(int((F.oracle_run(oracle_mod, r).align_field("is_dud") != 0).sum()) for r in F.ROWS)
    invalid = sum(int((F.oracle_run(oracle_mod, r).align_field("valid") == 0).sum()) for r in F.ROWS)
    assert duds > 0 and invalid > 0
