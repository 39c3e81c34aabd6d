"""Model.retrieve_scene (jur_retrieve_scene_host) where the passes that its loop cuts anew, on the rays that remain once
slices have ended, are larger than any pass of the first cut -- in slots and in block columns.  The pass arrays, the
forward model's workspace and the block-column region of the call are sized by jur_scene_pass_reserve for exactly these
passes; sized by the first cut they are written beyond their ends.

Every case runs the retrieval twice, each time on a model of its own (the arrays of a model only grow: one that has served
a larger call hides arrays that are too small): once with the default cap, the whole scene in one pass, and once with a
cap searched on the host with lib.scene_passes from the first run's history, such that a re-cut pass exceeds the first
cut.  No output may depend on the cap: everything is compared bit for bit."""
import numpy as np
import pytest
import sequences
from test_scene_jacobian_gpu import bits, formod_on, fresh_formod
from test_scene_normal_gpu import inputs, interleaved
import test_scene_retrieve_gpu as T
import test_scene_fov_gpu as F
import test_prior_full_gpu as P

pytestmark = pytest.mark.gpu
STALLS = 1                                                              # the slice made to stall: its y is F(first guess)
COMPARED = T.HISTORY + ("h_work", "x", "rad", "tau", "tp", "np") + T.PER_SLICE


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def run(hip, case, geom, y, weight, mode, settings, prior=None, cap=0, setup=None):
    """retrieve_scene with full history on a fresh model, and formod_host on that model afterwards"""
    s = dict(settings)
    mi, fac = s.pop("max_iter"), s.pop("fac")
    pk = dict(prior_ivar=prior[0], prior_xa=prior[1]) if prior else {}
    model = hip.Model(case.ctl, case.lib_tables())
    try:
        model.set_atm(case.atm)
        if setup:
            setup(model)
        out = model.retrieve_scene(case.atm, geom, y, weight, mi, fac, mode=mode, history=True, max_rays_per_pass=cap, **s, **pk)
        out["after"] = formod_on(model, geom)
    finally:
        model.close()
    return out


def recuts(out):
    """the rays of every distinct set of slices that took part in an iteration after a slice had ended, as masks"""
    sid = out["sid"]
    seen, masks = set(), []
    for part in out["h_accept"] >= 0:
        if part.any() and not part.all() and part.tobytes() not in seen:
            seen.add(part.tobytes())
            masks.append((sid >= 0) & part[np.maximum(sid, 0)])
    return masks


def rowptr_of(widths):
    return np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)


def grown(hip, out, nlam, cap, time=None):
    """how many of the re-cuts have, under this cap, a pass with more slots than every pass of either kind of the first
    cut and more block columns than every pass of the first cut"""
    widths = np.diff(out["rowptr"])
    _, slots, cols = hip.scene_passes(out["rowptr"], cap, time)
    slots = max(slots, hip.trial_passes(len(widths), nlam, cap, time)[1])
    count = 0
    for keep in recuts(out):
        _, s2, c2 = hip.scene_passes(rowptr_of(widths[keep]), cap, None if time is None else time[keep])
        count += s2 > slots and c2 > cols
    return count


def searched_cap(hip, out, nlam, time=None):
    """the cap from 2 up to the scene's total under which most re-cuts grow (the smallest such), or None"""
    total = int(out["rowptr"][-1]) + len(out["sid"])
    counts = [grown(hip, out, nlam, cap, time) for cap in range(2, total + 1)]
    return 2 + int(np.argmax(counts)) if max(counts) > 0 else None


def check(hip, case, geom, whole, capped, cap, nlam, time=None):
    assert cap is not None and cap != 1 and grown(hip, whole, nlam, cap, time) >= 1, "no cap makes a re-cut pass exceed the first cut"
    slots, cols = hip.scene_pass_reserve(whole["rowptr"], cap, nlam, time)
    assert slots < int(whole["rowptr"][-1]) + len(geom), "the reserve of the capped run is not the whole scene"
    for f in COMPARED:
        bits(capped[f], whole[f], "%s, passes of %d" % (f, cap))
    T.same_atm(hip, capped["atm"], whole["atm"])
    assert grown(hip, capped, nlam, cap, time) >= 1                     # (the capped run took the same course)
    sequences.same_bits(capped["after"], fresh_formod(hip, case, capped["atm"], geom), "the model of the capped run holds atm_ret")
    print("RECUT cap %d of %d slots: %d of %d re-cuts exceed the first cut; reserve %d slots, %d columns"
          % (cap, int(whole["rowptr"][-1]) + len(geom), grown(hip, whole, nlam, cap, time), len(recuts(whole)), slots, cols))


def stalled_inputs(hip, order=None):
    """the "ragged" scene with slice STALLS unable to move, the rays in `order`"""
    case, geom, y, weight = inputs(hip, "ragged")
    lay = T.layout(hip, "ragged")[0]
    rays = lay["sid"] == STALLS
    y2 = y.copy()
    y2[rays] = fresh_formod(hip, case, case.atm, geom[rays])["rad"]
    order = np.arange(len(geom)) if order is None else order
    return case, geom[order], y2[order], weight[order], rays[order]


def both(hip, case, geom, y, weight, mode, settings, time=None, **kw):
    nlam = len(settings["fac"])
    whole = run(hip, case, geom, y, weight, mode, settings, **kw)
    cap = searched_cap(hip, whole, nlam, time)
    assert cap is not None, "no cap makes a re-cut pass exceed the first cut"
    capped = run(hip, case, geom, y, weight, mode, settings, cap=cap, **kw)
    check(hip, case, geom, whole, capped, cap, nlam, time)
    return whole


# ---- (a) one slice stalls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_a_stalled_slice(hip, mode):
    case, geom, y2, weight, rays = stalled_inputs(hip)
    lay, iq, ip, x0 = T.layout(hip, "ragged")
    prior = T.seeded_prior(hip, "ragged", lay, x0) if mode == hip.DAMP_PRIOR else None
    whole = both(hip, case, geom, y2, weight, mode, T.FLOW, prior=prior)
    assert whole["state"][STALLS] == hip.RET_STALLED and whole["iters"][STALLS] == 3
    assert len(recuts(whole)) == 1 and np.array_equal(recuts(whole)[0], (lay["sid"] >= 0) & ~rays)


# ---- (b) slices converge at different iterations ----------------------------------------------------------------------------
def test_slices_that_converge_in_turn(hip):
    case, geom, y, weight = inputs(hip, "ragged")
    settings = dict(T.FLOW, tol=0.5, max_iter=8)
    nlam = len(settings["fac"])
    whole = run(hip, case, geom, y, weight, 0, settings)
    cap = searched_cap(hip, whole, nlam)
    if cap is None:                                                     # (the rays dealt out in turn: other neighbours)
        order = interleaved(T.layout(hip, "ragged")[0]["sid"])
        geom, y, weight = geom[order], y[order], weight[order]
        whole = run(hip, case, geom, y, weight, 0, settings)
        cap = searched_cap(hip, whole, nlam)
    assert cap is not None, "no cap makes a re-cut pass exceed the first cut"
    assert len(recuts(whole)) >= 2, "the passes are re-cut in one iteration only"
    capped = run(hip, case, geom, y, weight, 0, settings, cap=cap)
    check(hip, case, geom, whole, capped, cap, nlam)
    assert np.any(whole["state"] == hip.RET_CONVERGED)


# ---- (c) with a field of view: passes extended to the end of a scan ---------------------------------------------------------
def test_a_stalled_slice_under_a_field_of_view(hip):
    case, geom, y, weight, lay = F.scene(hip)[:5]
    rays = lay["sid"] == STALLS
    y2 = y.copy()
    y2[rays] = F.convolved(hip, case, case.atm, geom)["rad"][rays]
    time = np.ascontiguousarray(geom[:, 0])
    whole = both(hip, case, geom, y2, weight, 0, T.FLOW, time=time, setup=lambda m: m.set_fov(F.DZ, F.W))
    assert whole["state"][STALLS] == hip.RET_STALLED and len(recuts(whole)) == 1
    final = F.convolved(hip, case, whole["atm"], geom)
    for f in ("rad", "tau"):
        bits(whole[f], final[f], "%s against formod_host + fov_apply on atm_ret" % f)


# ---- (d) with a full prior precision ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_a_stalled_slice_with_a_full_prior_precision(hip, mode):
    case, geom, y2, weight, rays = stalled_inputs(hip)
    lay, iq, ip, x0 = T.layout(hip, "ragged")
    pc, r, xa = P.scene_prior(hip, "ragged")
    xa2 = xa.copy()
    xa2[T.slice_mask(lay, STALLS)] = x0[T.slice_mask(lay, STALLS)]
    whole = both(hip, case, geom, y2, weight, mode, T.FLOW, prior=(r, xa2),
                 setup=lambda m: m.set_prior_precision(lay["wptr"], pc["R"]))
    assert whole["state"][STALLS] == hip.RET_STALLED and len(recuts(whole)) == 1
    assert np.all(whole["prior"][np.arange(len(whole["prior"])) != STALLS] > 0)


# ---- (e) the rays dealt out in turn -----------------------------------------------------------------------------------------
def test_a_stalled_slice_with_interleaved_rays(hip):
    order = interleaved(T.layout(hip, "ragged")[0]["sid"])
    assert not np.array_equal(order, np.arange(len(order)))
    case, geom, y2, weight, rays = stalled_inputs(hip, order)
    whole = both(hip, case, geom, y2, weight, 0, T.FLOW)
    stalled = int(whole["sid"][np.flatnonzero(rays)[0]])
    assert whole["state"][stalled] == hip.RET_STALLED and len(recuts(whole)) == 1
