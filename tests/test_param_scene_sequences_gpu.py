"""What Model.param_scene leaves in a model (the buffer beside the slab of the scene entries, the slab itself, the
retrieval windows it borrows for its second phase, the stacked atmosphere) must not show in any later result, and what
earlier calls left must not show in its own: one long-lived model runs param_scene, retrieve_scene, param_scene with other
parameter windows and gain_scene, and every step answers BIT FOR BIT as a fresh model does (the manner of
tests/test_sequences_gpu.py, on the scene entries)."""
import numpy as np
import pytest
from test_scene_jacobian_gpu import bits, per_time_stamp, scene_case
from test_scene_param_gpu import copy_ctl, no_windows, window_fields
from test_scene_param_scene_gpu import entry, new_model, problem, same, windows_t, windows_x

pytestmark = pytest.mark.gpu
SETTINGS = dict(max_iter=2, fac=(0.1, 1.0, 10.0), lam0=10.0, lam_min=1e-6, lam_max=100.0, tol=0.0)


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def test_a_long_lived_model_answers_as_fresh_ones(hip):
    case = scene_case("ragged")
    geom = per_time_stamp(case.geom, 6)
    ctl_x, ctl_t = windows_x(case), windows_t(case)
    ctl_q = copy_ctl(case.ctl)                                      # other parameters: the pressure and another gas, wider
    no_windows(ctl_q)
    ctl_q.retp_zmin, ctl_q.retp_zmax = 5.0, 60.0
    ctl_q.retq_zmin[0], ctl_q.retq_zmax[0] = 0.0, 50.0

    def steps(model, p_t, p_q):
        yield "param_scene", lambda: entry(model, case, geom, ctl_t, p_t, want_gain=True, want_kb=True, max_rays_per_pass=500)
        yield "retrieve_scene", lambda: model.retrieve_scene(case.atm, geom, p_t["y"], p_t["weight"], prior_ivar=p_t["prior"],
                                                             prior_xa=xa, rad_in=p_t["rad_in"], **SETTINGS)
        yield "param_scene with other windows", lambda: entry(model, case, geom, ctl_q, p_q, want_kb=True)
        yield "gain_scene", lambda: model.gain_scene(case.atm, geom, p_t["y"], p_t["weight"], prior_ivar=p_t["prior"], want_gain=True,
                                                     rad_in=p_t["rad_in"])

    def strip(out):
        return {k: v for k, v in out.items() if k != "atm"}

    setup = new_model(hip, case, ctl_x)
    try:
        p_t = problem(hip, setup, case, geom, ctl_t)
        p_q = problem(hip, setup, case, geom, ctl_q, ncov=0)
        lay = hip.scene_slices(ctl_x, case.atm, geom[:, 0])
        xa = np.concatenate([np.array([case.atm.q[2][i] for i in hip.scene_elements(ctl_x, case.atm, int(f), int(l))["ip"]])
                             for f, l in zip(lay["sfirst"], lay["slen"])])
    finally:
        setup.close()
    assert np.any(np.diff(p_q["lay"]["bwptr"]) != np.diff(p_t["lay"]["bwptr"]))
    fresh = []
    for i in range(4):
        m = new_model(hip, case, ctl_x)
        try:
            fresh.append(list(steps(m, p_t, p_q))[i][1]())
        finally:
            m.close()
    model = new_model(hip, case, ctl_x)
    try:
        for (what, run), ref in zip(steps(model, p_t, p_q), fresh):
            got = run()
            same(strip(got), strip(ref), "%s on the long-lived model" % what)
            if "atm" in ref:
                for f in ("p", "t"):
                    bits(np.ctypeslib.as_array(getattr(got["atm"], f)), np.ctypeslib.as_array(getattr(ref["atm"], f)), "atm.%s" % f)
                bits(np.ctypeslib.as_array(got["atm"].q), np.ctypeslib.as_array(ref["atm"].q), "atm.q")
            assert window_fields(model.ret_windows()) == window_fields(ctl_x), what
    finally:
        model.close()
    assert fresh[0]["sigma_param"].max() > 0 and fresh[2]["sigma_param"].max() > 0 and np.any(fresh[1]["iters"] > 0)
