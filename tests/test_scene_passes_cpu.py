"""jur_scene_passes, jur_trial_passes and jur_scene_pass_reserve (host arithmetic of the library, no GPU): how the scene
entries cut a call into passes, and what jur_retrieve_scene_host allocates for the passes that its loop cuts anew on the
rays that remain once slices have ended.

The cuts are held to their properties and to a restatement in numpy (running sums and np.searchsorted in place of the
library's ray-by-ray loop).  The reserve is held from both sides: every pass of either kind on every set of remaining
rays fits in it, and it stays within what the cap, the largest ray or scan and the whole call allow."""
import itertools
import numpy as np
import pytest
from jurassic_hip import lib

NAMED = dict(widths=[3, 5, 4, 4, 6, 7, 6], sid=[0, 1, 2, 0, 1, 0, 1], cap=9, ended=(1,))


def rowptr(widths):
    return np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)


def scan_ends(time):
    """one past the last ray of the scan (the maximal run of equal time stamps) of every ray"""
    n = len(time)
    last = np.flatnonzero(np.append(time[1:] != time[:-1], True)) + 1
    return last[np.searchsorted(last, np.arange(n), side="right")]


def cut(slots, cap, time=None):
    """passes over rays of `slots` slots each: as many rays as stay within cap, one at least, then to the end of the scan"""
    run = np.concatenate([[0], np.cumsum(slots)])
    end = scan_ends(np.asarray(time)) if time is not None else None
    out, r0, n = [0], 0, len(slots)
    while r0 < n:
        r1 = max(int(np.searchsorted(run, run[r0] + cap, side="right")) - 1, r0 + 1)
        if end is not None:
            r1 = int(end[r1 - 1])
        out.append(r1)
        r0 = r1
    return np.array(out, dtype=np.int64)


def trial_cut(nr, ntrial, cap, time=None):
    """max(cap // ntrial, 1) rays a pass whatever they are: the cut of rays of ntrial slots under a cap of whole rays"""
    return cut(np.full(nr, ntrial), max(cap // ntrial, 1) * ntrial, time)


def sizes(pas, per_ray):
    run = np.concatenate([[0], np.cumsum(per_ray)])
    return run[pas[1:]] - run[pas[:-1]]


def check_cut(pas, slots, cap, time, what):
    n = len(slots)
    assert pas[0] == 0 and pas[-1] == n and np.all(np.diff(pas) > 0), (what, "the passes tile 0..nr")
    got = sizes(pas, slots)
    for p, (r0, r1) in enumerate(zip(pas[:-1], pas[1:])):
        if time is None:
            assert got[p] <= cap or r1 - r0 == 1, (what, p, "beyond the cap and not a single ray")
        else:
            end = scan_ends(time)
            assert end[r1 - 1] == r1, (what, p, "a scan is split")
            assert r0 == 0 or end[r0 - 1] == r0, (what, p, "a scan is split")
            # before it was extended the pass ended inside its last scan: that part is within the cap or is one ray
            first_of_last = max(int(np.flatnonzero(end == r1)[0]), r0)
            # (a pass of one scan is a ray within the cap or beyond it, extended)
            assert first_of_last == r0 or slots[r0:first_of_last + 1].sum() <= cap, (what, p, "beyond the cap before its last scan ends")


def seeded_widths(rng, n, cap_like):
    w = rng.integers(0, 8, n)
    w[rng.integers(n)] = 0
    w[rng.integers(n)] = cap_like + 3                                   # one ray wider than the middle cap
    return w


def seeded_times(rng, n):
    """scans of 1 to 5 rays, ascending time stamps"""
    lengths = []
    while sum(lengths) < n:
        lengths.append(int(rng.integers(1, 6)))
    return np.repeat(np.arange(len(lengths), dtype=np.float64), lengths)[:n]


@pytest.mark.parametrize("with_time", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_cutting(seed, with_time):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(9, 40))
    mid = 11
    w = seeded_widths(rng, n, mid)
    rp = rowptr(w)
    time = seeded_times(rng, n) if with_time else None
    total = int(rp[-1]) + n
    assert (w == 0).any() and w.max() + 1 > mid
    for cap in (1, 2, mid, total, total + 1):
        pas, nmax, kmax = lib.scene_passes(rp, cap, time)
        check_cut(pas, w + 1, cap, time, ("scene", seed, cap))
        assert np.array_equal(pas, cut(w + 1, cap, time)), (seed, cap)
        assert nmax == sizes(pas, w + 1).max() and kmax == sizes(pas, w).max(), (seed, cap)
        if cap >= total:
            assert len(pas) == 2
        for ntrial in (1, 3, 8):
            tpas, tmax = lib.trial_passes(n, ntrial, cap, time)
            check_cut(tpas, np.full(n, ntrial), max(cap, ntrial), time, ("trial", seed, cap, ntrial))
            assert np.array_equal(tpas, trial_cut(n, ntrial, cap, time)), (seed, cap, ntrial)
            assert tmax == np.diff(tpas).max() * ntrial, (seed, cap, ntrial)
            if time is None:                                            # whole rays under the cap, and as many as fit
                assert np.all(np.diff(tpas)[:-1] == max(cap // ntrial, 1)) and np.diff(tpas)[-1] <= max(cap // ntrial, 1)


def test_cutting_edges():
    pas, nmax, kmax = lib.scene_passes([0], 5)
    assert list(pas) == [0] and (nmax, kmax) == (0, 0)
    pas, nmax = lib.trial_passes(0, 3, 5)
    assert list(pas) == [0] and nmax == 0
    assert lib.scene_pass_reserve([0], 5, 3) == (0, 0)
    assert lib.scene_pass_reserve([0, 0], 5, 3) == (3, 0)               # one ray without elements: itself, and its trials
    for call in (lambda: lib.scene_passes([0, 1], 0), lambda: lib.trial_passes(2, 0, 4), lambda: lib.trial_passes(2, 1, 0),
                 lambda: lib.scene_pass_reserve([0, 1], 0, 1), lambda: lib.scene_pass_reserve([0, 1], 4, 0)):
        with pytest.raises(lib.JurassicError, match=r"error %d: jur_\w+: bad arguments" % lib.EINVAL):
            call()
    with pytest.raises(lib.JurassicError, match=r"error %d: jur_scene_passes: a pass of 2\^31 slots" % lib.EINVAL):
        lib.scene_passes([0, 2 ** 31 - 1], 7)                           # 2^31 - 1 elements and the ray itself
    assert lib.scene_passes([0, 2 ** 31 - 2], 7)[1:] == (2 ** 31 - 1, 2 ** 31 - 2)
    with pytest.raises(lib.JurassicError, match=r"error %d: jur_trial_passes: a pass of 2\^31 slots" % lib.EINVAL):
        lib.trial_passes(4, 2 ** 30, 1, np.zeros(4))                    # a scan of four rays of 2^30 trials each


# ---- the reserve ---------------------------------------------------------------------------------------------------------
def single_rays(seed):
    """rays of 3 to 8 groups of one ray each, dealt to 2 to 5 slices at random; a ray of width 0 is in no slice"""
    rng = np.random.default_rng(seed)
    n, ns = int(rng.integers(3, 9)), int(rng.integers(2, 6))
    while True:                                                         # (until two slices have rays)
        w = rng.integers(0, 8, n)
        sid = rng.integers(0, ns, n)
        sid[w == 0] = -1
        if len(set(sid[sid >= 0].tolist())) >= 2:
            return w, sid, None


def scans(seed):
    """3 to 8 scans of 2 to 6 rays in 2 to 5 slices: a scan's rays share its time stamp, its slice and so its width"""
    rng = np.random.default_rng(seed)
    n, ns = int(rng.integers(3, 9)), int(rng.integers(2, 6))
    lengths = rng.integers(2, 7, n)
    while True:
        sid = rng.integers(0, ns, n)
        w = rng.integers(0, 8, ns)[sid]
        sid = np.where(w == 0, -1, sid)
        if len(set(sid[sid >= 0].tolist())) >= 2:
            return np.repeat(w, lengths), np.repeat(sid, lengths), np.repeat(np.arange(n, dtype=np.float64), lengths)


def remaining(sid):
    """the rays the loop can be left with: those of the slices that have not ended, for every proper non-empty set of
    ended slices -- and for none ended where rays without state elements drop out of the first iteration already"""
    live = sorted(set(sid[sid >= 0].tolist()))
    for k in range(0 if (sid < 0).any() else 1, len(live)):
        for ended in itertools.combinations(live, k):
            yield ended, (sid >= 0) & ~np.isin(sid, ended)


def overflows(reserve, w, sid, time, ntrials=(1, 3)):
    """(cap, ntrial, ended, kind, needed, reserved) of every re-cut pass that does not fit what `reserve` gives"""
    rp = rowptr(w)
    bad = []
    subsets = [(ended, keep, rowptr(w[keep]), None if time is None else time[keep]) for ended, keep in remaining(sid)]
    for cap in range(1, int(rp[-1]) + len(w) + 2):
        cuts = [(ended, int(keep.sum()), tk) + lib.scene_passes(rk, cap, tk)[1:] for ended, keep, rk, tk in subsets]
        for ntrial in ntrials:
            slots, cols = reserve(rp, cap, ntrial, time)
            for ended, n, tk, nmax, kmax in cuts:
                tmax = lib.trial_passes(n, ntrial, cap, tk)[1]
                for kind, need, have in (("slots", nmax, slots), ("columns", kmax, cols), ("trial slots", tmax, slots)):
                    if need > have:
                        bad.append((cap, ntrial, ended, kind, need, have))
    return bad


def first_cut_only(rp, cap, ntrial, time):
    """what the entry reserved before jur_scene_pass_reserve, without a field of view: the largest pass of the first cut"""
    _, nmax, kmax = lib.scene_passes(rp, cap, time)
    return max(nmax, lib.trial_passes(len(rp) - 1, ntrial, cap, time)[1]), kmax


CASES = [(single_rays, s) for s in range(24)] + [(scans, s) for s in range(8)]


@pytest.mark.parametrize("make,seed", CASES, ids=["%s-%d" % (m.__name__, s) for m, s in CASES])
def test_every_recut_pass_fits_the_reserve(make, seed):
    w, sid, time = make(seed)
    assert len(set(sid[sid >= 0].tolist())) >= 2
    bad = overflows(lib.scene_pass_reserve, w, sid, time)
    assert not bad, (len(bad), bad[:5])


def test_the_first_cut_alone_is_too_small():
    """the gap this file closes: sized by the first cut, re-cut passes of rays without time stamps overflow"""
    found = sum(len(overflows(first_cut_only, *single_rays(s))) for s in range(24))
    assert found > 0


def limits(w, cap, ntrial, time):
    """what the reserve may cost at most, in slots and in columns"""
    n = len(w)
    all_slots, all_cols = int(w.sum()) + n, int(w.sum())
    if time is None:
        # a pass within the cap (one slot of it is no column) or one ray; a trial pass of whole rays within the cap, or of
        # one ray
        slots = max(cap, int(w.max()) + 1, ntrial)
        cols = max(cap - 1, int(w.max()))
    else:
        # the cap and one more scan; a trial pass takes cap // ntrial rays, one ray whatever the cap, and one more scan
        ends = np.flatnonzero(np.append(time[1:] != time[:-1], True)) + 1
        starts = np.concatenate([[0], ends[:-1]])
        scan_w = np.array([w[a:b].sum() for a, b in zip(starts, ends)])
        scan_n = ends - starts
        slots = max(cap + int((scan_w + scan_n).max()), cap + ntrial + int(scan_n.max()) * ntrial)
        cols = cap + int(scan_w.max())
    return min(slots, max(all_slots, n * ntrial)), min(cols, all_cols)


@pytest.mark.parametrize("make,seed", CASES[::3], ids=["%s-%d" % (m.__name__, s) for m, s in CASES[::3]])
def test_the_reserve_stays_a_bound_on_memory(make, seed):
    w, sid, time = make(seed)
    rp = rowptr(w)
    total = int(rp[-1]) + len(w)
    for cap in range(1, total + 2):
        for ntrial in (1, 3):
            slots, cols = lib.scene_pass_reserve(rp, cap, ntrial, time)
            most = limits(w, cap, ntrial, time)
            assert slots <= most[0] and cols <= most[1], (cap, ntrial, (slots, cols), most)
            if cap >= total and (time is None or cap // ntrial >= len(w)):   # one pass of either kind: exactly those
                assert (slots, cols) == (max(total, min(max(cap // ntrial, 1), len(w)) * ntrial), int(rp[-1]))
            first = first_cut_only(rp, cap, ntrial, time)
            assert slots >= first[0] and cols >= first[1], (cap, ntrial, (slots, cols), first)


def test_the_named_case():
    w, sid = np.array(NAMED["widths"]), np.array(NAMED["sid"])
    cap = NAMED["cap"]
    rp = rowptr(w)
    pas, nmax, kmax = lib.scene_passes(rp, cap)
    assert list(pas) == list(range(8)) and (nmax, kmax) == (8, 7)      # no two neighbours fit in 9 slots
    keep = ~np.isin(sid, NAMED["ended"])
    assert list(w[keep]) == [3, 4, 4, 7]
    again, nmax2, kmax2 = lib.scene_passes(rowptr(w[keep]), cap)
    assert sizes(again, w[keep] + 1)[0] == 9 and nmax2 == 9
    slots, cols = lib.scene_pass_reserve(rp, cap, 1)                    # (one trial a ray: no trial pass has 8 slots)
    assert slots >= 9 and cols >= kmax2
    assert first_cut_only(rp, cap, 1, None)[0] == 8
    print("PASSES named case: first cut %d slots, re-cut %d slots, reserve %d slots and %d columns" % (nmax, nmax2, slots, cols))
