"""jur_param_scene_host without a GPU: the library exports the entry, the binding's struct mirrors have the sizes the
library reports, and the host arithmetic of its passes (jur_param_pass_range, jur_param_pass_maps: the stretch of a
slice's ascending ray list inside a pass, the tiles of C a pass reaches) agrees with a few lines of numpy on hand-made
layouts: interleaved slices, a slice with no ray in the pass, a pass of one ray."""
import ctypes as C
import numpy as np
import pytest


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    return lib


LP, IP = C.POINTER(C.c_long), C.POINTER(C.c_int)


def lists(sid, nslice):
    """sptr, srays as jur_scene_rays_by_slice makes them"""
    rays = [np.flatnonzero(sid == q) for q in range(nslice)]
    sptr = np.concatenate([[0], np.cumsum([len(r) for r in rays])]).astype(np.int64)
    srays = np.concatenate(rays + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return sptr, np.ascontiguousarray(srays if len(srays) else np.zeros(1, dtype=np.int32))


def pass_range(hip, sptr, srays, s, r0, r1):
    lo, hi = C.c_long(-1), C.c_long(-1)
    hip.lib().jur_param_pass_range(sptr.ctypes.data_as(LP), srays.ctypes.data_as(IP), s, r0, r1, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def pass_maps(hip, wptr, bwptr, sptr, srays, sid, r0, r1, mark):
    ntile = sum(-(-int(w) // 64) * -(-int(b) // 64) for w, b in zip(np.diff(wptr), np.diff(bwptr)))
    pmap = np.full(5 * max(ntile, 1), -7, dtype=np.int32)
    n = hip.lib().jur_param_pass_maps(wptr.ctypes.data_as(LP), bwptr.ctypes.data_as(LP), sptr.ctypes.data_as(LP),
                                      srays.ctypes.data_as(IP), sid.ctypes.data_as(IP), r0, r1, mark.ctypes.data_as(LP),
                                      pmap.ctypes.data_as(IP))
    assert np.all(pmap[5 * n:] == -7)
    return pmap[:5 * n].reshape(n, 5)


def expected_maps(wptr, bwptr, sptr, srays, sid, r0, r1):
    out, seen = [], set()
    for r in range(r0, r1):
        q = int(sid[r])
        if q < 0 or q in seen:
            continue
        seen.add(q)
        mine = srays[sptr[q]:sptr[q + 1]]
        lo = int(sptr[q] + np.searchsorted(mine, r0))
        hi = int(sptr[q] + np.searchsorted(mine, r1))
        w, wb = int(wptr[q + 1] - wptr[q]), int(bwptr[q + 1] - bwptr[q])
        out += [(q, i0, j0, lo, hi) for i0 in range(0, w, 64) for j0 in range(0, wb, 64)]
    return np.array(out, dtype=np.int32).reshape(len(out), 5)


def test_exports_and_struct_sizes(hip):
    L = hip.lib()
    for name in ("jur_param_scene_host", "jur_param_scene_abi_sizes", "jur_model_scene_bytes", "jur_param_pass_range",
                 "jur_param_pass_maps"):
        assert hasattr(L, name), name
    out = (C.c_size_t * 2)()
    L.jur_param_scene_abi_sizes(out)
    assert list(out) == [C.sizeof(hip.ParamSceneIn), C.sizeof(hip.ParamSceneOut)] == [32, 24]
    assert [getattr(hip.ParamSceneIn, f).offset for f in ("ctl_b", "rowptr_b", "bwptr", "in_")] == [0, 8, 16, 24]
    assert [getattr(hip.ParamSceneOut, f).offset for f in ("out", "kb", "weight_eff")] == [0, 8, 16]
    assert hasattr(hip.Model, "param_scene")
    assert L.jur_model_scene_bytes(None) == 0


def test_named_passes(hip):
    # three slices interleaved, a leading ray without a slice; slice 1 has no parameters, slice 2 two tiles across
    sid = np.array([-1, 0, 2, 0, 1, 2, 0, 2, 2], dtype=np.int32)
    wptr = np.array([0, 3, 5, 70], dtype=np.int64)
    bwptr = np.array([0, 6, 6, 71], dtype=np.int64)
    sptr, srays = lists(sid, 3)
    assert list(sptr) == [0, 3, 4, 8] and list(srays) == [1, 3, 6, 4, 2, 5, 7, 8]
    assert pass_range(hip, sptr, srays, 0, 0, 4) == (0, 2)
    assert pass_range(hip, sptr, srays, 0, 4, 6) == (2, 2)                   # no ray of slice 0 in the pass: empty
    assert pass_range(hip, sptr, srays, 2, 6, 9) == (6, 8)
    assert pass_range(hip, sptr, srays, 2, 5, 6) == (5, 6)                   # a pass of one ray
    mark = np.zeros(3, dtype=np.int64)
    got = pass_maps(hip, wptr, bwptr, sptr, srays, sid, 0, 4, mark)
    assert got.tolist() == [[0, 0, 0, 0, 2], [2, 0, 0, 4, 5], [2, 0, 64, 4, 5], [2, 64, 0, 4, 5], [2, 64, 64, 4, 5]]
    got = pass_maps(hip, wptr, bwptr, sptr, srays, sid, 4, 5, mark)          # the ray of slice 1 alone: wb = 0, no tile
    assert got.shape == (0, 5)
    got = pass_maps(hip, wptr, bwptr, sptr, srays, sid, 5, 9, mark)
    assert got.tolist() == [[2, 0, 0, 5, 8], [2, 0, 64, 5, 8], [2, 64, 0, 5, 8], [2, 64, 64, 5, 8], [0, 0, 0, 2, 3]]
    got = pass_maps(hip, wptr, bwptr, sptr, srays, sid, 0, 1, np.zeros(3, dtype=np.int64))   # a ray without a slice alone
    assert got.shape == (0, 5)


def test_seeded_layouts_against_numpy(hip):
    rng = np.random.default_rng(23)
    for trial in range(60):
        nslice, nr = int(rng.integers(1, 7)), int(rng.integers(1, 50))
        sid = rng.integers(-1, nslice, nr).astype(np.int32)
        wptr = np.concatenate([[0], np.cumsum(rng.choice([1, 63, 64, 65, 130], nslice))]).astype(np.int64)
        bwptr = np.concatenate([[0], np.cumsum(rng.choice([0, 1, 64, 65, 130], nslice))]).astype(np.int64)
        sptr, srays = lists(sid, nslice)
        mark = np.zeros(nslice, dtype=np.int64)
        cuts = np.unique(np.concatenate([[0, nr], rng.integers(0, nr + 1, int(rng.integers(0, 6)))]))
        covered = {q: [] for q in range(nslice)}
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            got = pass_maps(hip, wptr, bwptr, sptr, srays, sid, int(r0), int(r1), mark)
            assert np.array_equal(got, expected_maps(wptr, bwptr, sptr, srays, sid, int(r0), int(r1))), (trial, r0, r1)
            for q in range(nslice):
                lo, hi = pass_range(hip, sptr, srays, q, int(r0), int(r1))
                covered[q] += list(range(lo, hi))
        for q in range(nslice):                                              # the passes take every ray of a slice once, in order
            assert covered[q] == list(range(int(sptr[q]), int(sptr[q + 1]))), (trial, q)
