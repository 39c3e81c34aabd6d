"""The GPU paths on ragged multi-profile scenes across the globe (synth.SCENES) against the CPU oracle, and against
each other bit for bit where they must agree: profiles of their own length, range, order and place, rays at each of
them in any azimuth, over the poles and across the dateline, and ray time stamps that match no profile.

Tolerances as tests/test_parity_gpu.py: 1e-9 relative on radiances, common.tau_atol on transmittances, LOS point
counts exact.  Tangent points are compared as Cartesian positions (0.1 mm): near a pole or the dateline a difference
of longitudes says nothing."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest
import common
from jurassic_hip import abi, synth

pytestmark = pytest.mark.gpu
RTOL = 1e-9
SCENES = sorted(synth.SCENES)
ARRANGEMENTS = ("fused", "batched", "batched_grouped")


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


def scene_case(name, sort_by_time=False, **ctl_kw):
    case = common.limb_case(**ctl_kw)
    if name.endswith("_ext"):         # the scene with an extinction that varies with altitude (regridded from the base)
        common.extinction_profile(case.atm)
        name = name[:-len("_ext")]
    atm, geom, _ = synth.scene(name, case.ctl, case.atm)
    if sort_by_time:                  # whole workgroups of the fused kernel share one slice: its LDS copy is made
        geom = geom[np.argsort(geom[:, 0], kind="stable")]
    case.atm, case.geom = atm, geom
    return case


_oracle = {}


def oracle_result(oracle, name, case, key=()):
    k = (name,) + tuple(key)
    if k not in _oracle:
        _oracle[k] = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom)
    return _oracle[k]


def run(hip, case, arrangement="fused", atm=None, rays_per_group=0):
    model = hip.Model(case.ctl, case.lib_tables())
    if arrangement != "fused":
        model.set_pencil(0)
    elif rays_per_group:
        model.set_pencil(10_000, rays_per_group)
    if arrangement == "batched_grouped":
        hip.tune_combine(4, 8, 0)
    try:
        model.set_atm(case.atm if atm is None else atm)
        return model.formod_host(case.geom)
    finally:
        if arrangement == "batched_grouped":
            hip.tune_combine(-1, 8, 1_000_000)
        model.close()


def assert_parity(out, ref, rtol=RTOL):
    assert np.array_equal(out["np"], ref["np"])
    fin = np.isfinite(ref["rad"])
    assert np.array_equal(fin, np.isfinite(out["rad"]))
    assert common.rel_err(out["rad"][fin], ref["rad"][fin]).max(initial=0) < rtol
    terr = np.abs(out["tau"] - ref["tau"])
    assert np.all(terr[fin] <= (rtol * np.abs(ref["tau"]) + common.tau_atol(ref["tau"]))[fin])
    assert np.abs(out["tp"][:, 0] - ref["tp"][:, 0]).max() < 1e-9
    d = np.linalg.norm(synth._cart(*out["tp"].T) - synth._cart(*ref["tp"].T), axis=1)
    assert d.max() < 1e-7                                    # km: 0.1 mm


def same_bits(a, b):
    for k in ("rad", "tau", "tp", "np"):
        assert np.array_equal(a[k], b[k], equal_nan=(k != "np")), k


@pytest.mark.parametrize("order", ["mixed", "by_time"])
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("name", SCENES)
def test_scene_against_oracle(hip, oracle, name, arrangement, order):
    """mixed: rays of all profiles in turn; by_time: sorted by time stamp, so that the workgroups of the fused kernel
    share one slice and it copies that slice to LDS (in lone_up the slice a one-point last profile joins: its copy
    must hold that point too, or the 0-60 km profile's rays enter at 60 km instead of 75)."""
    case = scene_case(name, sort_by_time=(order == "by_time"))
    ref = oracle_result(oracle, name, case, (order,))
    assert (ref["np"] > 1).sum() >= 25
    assert_parity(run(hip, case, arrangement), ref)


@pytest.mark.parametrize("name", SCENES)
def test_one_and_four_lanes_per_ray(hip, name):
    """The batched tracer with one lane per ray and with a quad of lanes per ray (one refraction probe each)."""
    case = scene_case(name)
    try:
        hip.tune_trace(1)
        one = run(hip, case, "batched")
        hip.tune_trace(4)
        four = run(hip, case, "batched")
    finally:
        hip.tune_trace(0)
    same_bits(one, four)


CHILD = r"""
import os, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, 'jurassic-gpu_amd'), os.path.join({root!r}, 'tests')]
import numpy as np, test_scenes_gpu as T
from jurassic_hip import lib
case = T.scene_case({name!r}, sort_by_time=True)
out = T.run(lib, case, "fused")
np.savez({path!r}, **out)
"""


@pytest.mark.parametrize("name", SCENES)
def test_pencil_profile_copy_on_and_off(hip, oracle, name, tmp_path):
    """The fused kernel with its LDS copy of the profile slice (made when every ray of a workgroup uses one slice: rays
    sorted by time stamp) and without (JUR_PENCIL_NO_ATM_LDS, read once per process: a child process).  at_cap has a
    slice of exactly the largest length that fits, over_cap one of one more."""
    case = scene_case(name, sort_by_time=True)
    on = run(hip, case, "fused")
    path = str(tmp_path / "off.npz")
    env = dict(os.environ, JUR_PENCIL_NO_ATM_LDS="1")
    subprocess.run([sys.executable, "-c", CHILD.format(root=common.ROOT, name=name, path=path)], env=env, check=True,
                   timeout=300)
    off = dict(np.load(path))
    same_bits(on, off)
    assert_parity(on, oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom))


@pytest.mark.parametrize("arrangement", ["fused", "batched"])
@pytest.mark.parametrize("name", ["ragged", "lone_up", "at_cap"])
def test_ray_order(hip, name, arrangement):
    """A permutation of the rays gives the permuted results bit for bit: rays sorted by slice (whole workgroups share
    one) against rays of all profiles mixed within every workgroup.  The fused kernel runs 16 rays per workgroup here
    (at ~200 rays it would pick 2 on its own), so that a shuffled workgroup holds rays of every profile."""
    case = scene_case(name, sort_by_time=True)
    a = run(hip, case, arrangement, rays_per_group=16)
    perm = np.random.default_rng(5).permutation(len(case.geom))
    case.geom = case.geom[perm]
    assert len(set(case.geom[:16, 0])) >= min(4, len(set(case.geom[:, 0])))     # one workgroup, many slices
    b = run(hip, case, arrangement, rays_per_group=16)
    same_bits({k: v[perm] for k, v in a.items()}, b)


def edited_atm(case, v):
    """case.atm for contribution variant v (v < ng: gas v alone, no extinction; v == ng: no gas)."""
    a = abi.atm_t()
    C.memmove(C.byref(a), C.byref(case.atm), C.sizeof(abi.atm_t))
    q, k = np.ctypeslib.as_array(a.q), np.ctypeslib.as_array(a.k)
    for g in range(case.ctl.ng):
        if g != v:
            q[g, :] = 0.0
    if v < case.ctl.ng:
        k[:, :] = 0.0
    return a


@pytest.mark.parametrize("hydz", [-999.0, 10.0])
@pytest.mark.parametrize("arrangement", ["fused", "batched"])
@pytest.mark.parametrize("name", ["ragged", "lone_ends", "lone_up", "short_last", "ragged_ext"])
def test_contributions(hip, oracle, name, arrangement, hydz):
    """formod_contrib_host: every variant against the oracle on the edited atmosphere.  With HYDZ >= 0 and H2O among
    the emitters the variants other than H2O's are one stacked call (time stamps shifted per copy), where every ray
    must meet the slice it has alone: the rays whose time stamps match no profile, those of the one-point profiles at
    the ends of lone_ends / lone_up (0.0, 5.0) and of the slices those join, and short_last's ray time stamp that
    locate_atm resolves to the two-level last profile."""
    case = scene_case(name, hydz=hydz)
    model = hip.Model(case.ctl, case.lib_tables())
    if arrangement != "fused":
        model.set_pencil(0)
    model.set_atm(case.atm)
    out = model.formod_contrib_host(case.geom)
    model.close()
    tb = case.oracle_tables(oracle)
    ref = oracle.formod_rays(case.ctl, case.atm, tb, case.geom)
    assert_parity(out, ref)
    for v in range(case.ctl.ng + 1):
        e = edited_atm(case, v)
        r = oracle.formod_rays(case.ctl, e, tb, case.geom)
        fin = np.isfinite(r["rad"])
        err = np.abs(out["rad_c"][v] - r["rad"])
        # a contribution far below the ray's total: the look-up's absolute ~1e-13 (see test_contrib_gpu.ORACLE_FLOOR)
        assert np.all((err <= RTOL * np.abs(r["rad"])) | (err <= 1e-14 * np.abs(ref["rad"]))), v
        terr = np.abs(out["tau_c"][v] - r["tau"])
        assert np.all(terr[fin] <= (RTOL * np.abs(r["tau"]) + common.tau_atol(r["tau"]))[fin]), v
    if name.endswith("_ext"):
        assert out["tau_c"][case.ctl.ng].min() < 0.9          # the extinction alone is not empty


def _obs(geom, nd):
    obs = abi.obs_t()
    obs.nr = len(geom)
    for k, name in enumerate(("time", "obsz", "obslon", "obslat", "vpz", "vplon", "vplat")):
        np.ctypeslib.as_array(getattr(obs, name))[:len(geom)] = geom[:, k]
    return obs


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("name", ["ragged", "lone_ends", "lone_up", "short_last"])
def test_jacobian(hip, oracle, name, arith):
    """Model.kernel (the perturbed atmospheres stacked as slices, one batched call) against the reference's loop of
    forward models (oracle.kernel), as test_parity_gpu.test_jacobian_matches_reference_kernel."""
    case = scene_case(name)
    c = case.ctl
    c.rett_zmin, c.rett_zmax = 10.0, 40.0
    c.retq_zmin[2], c.retq_zmax[2] = 15.0, 35.0
    geom = np.vstack([case.geom[case.geom[:, 0] == t][:6] for t in np.unique(case.geom[:, 0])])   # every time stamp
    obs_ref, obs = _obs(geom, 2), _obs(geom, 2)
    k_ref = oracle.kernel(c, case.atm, obs_ref, case.oracle_tables(oracle))
    model = hip.Model(c, case.lib_tables())
    model.set_arithmetic(hip.ARITH_EXACT if arith == "exact" else hip.ARITH_FAST)
    model.set_atm(case.atm)
    k = model.kernel(case.atm, obs)
    model.close()
    assert k.shape == k_ref.shape and k.shape[1] >= 40
    scale = np.abs(k_ref).max(axis=0)
    live = scale > 0
    assert live.sum() >= 25 and np.all(k[:, ~live] == 0)
    assert np.max(np.abs(k[:, live] - k_ref[:, live]) / scale[live]) < 1e-6
    n = obs.nr
    a, b = np.ctypeslib.as_array(obs.rad)[:n, :2], np.ctypeslib.as_array(obs_ref.rad)[:n, :2]
    assert common.rel_err(a, b).max() < RTOL


@pytest.mark.parametrize("name", ["ragged", "lone_up"])
def test_host_multi_entry(hip, name):
    """jur_formod_host_multi with the model listed 1 - 3 times: the rays dealt to the entries, bit-identical to one."""
    case = scene_case(name)
    one = run(hip, case)
    for count in (1, 2, 3):
        models = [hip.Model(case.ctl, case.lib_tables()) for _ in range(count)]
        hip.models_set_atm(models, case.atm)
        out = hip.formod_host_multi(models, case.geom)
        for m in models:
            m.close()
        same_bits(one, out)


def write_atm_tab(path, atm, ctl):
    n = atm.np
    cols = [np.ctypeslib.as_array(getattr(atm, f))[:n] for f in ("time", "z", "lon", "lat", "p", "t")]
    cols += [np.ctypeslib.as_array(atm.q)[g, :n] for g in range(ctl.ng)]
    cols += [np.ctypeslib.as_array(atm.k)[w, :n] for w in range(ctl.nw)]
    np.savetxt(path, np.column_stack(cols), fmt="%.17g")


@pytest.mark.parametrize("name", ["ragged", "lone_ends"])
def test_drop_in_atm_tab(hip, oracle, name, tmp_path):
    """The scene written as an atm.tab of several profiles, read back and passed through formod() and formod_pencil().
    The drop-in entry reads its tables once per process, as the reference does: the state an earlier test left is
    freed first (jur_dropin_finalize), so that this call reads this scene's files, and freed again afterwards."""
    from jurassic_hip import textio
    hip.dropin_finalize()
    case = scene_case(name)
    case.write_files(str(tmp_path), base="tbl")
    write_atm_tab(str(tmp_path / "atm.tab"), case.atm, case.ctl)
    atm = textio.read_atm(str(tmp_path / "atm.tab"), case.ctl)
    assert atm.np == case.atm.np
    t_ref = oracle.Tables(case.ctl.ng, case.ctl.nd)
    assert t_ref.read_ascii(case.ctl) == 0 and t_ref.planck_filt(case.ctl) == 0
    ref = oracle.formod_rays(case.ctl, atm, t_ref, case.geom)
    case.ctl.useGPU = 1
    obs = _obs(case.geom, 2)
    hip.formod(case.ctl, atm, obs)
    n = obs.nr
    rad = np.ctypeslib.as_array(obs.rad)[:n, :2]
    fin = np.isfinite(ref["rad"])
    assert np.array_equal(fin, np.isfinite(rad))
    assert common.rel_err(rad[fin], ref["rad"][fin]).max() < RTOL
    tp = np.column_stack([np.ctypeslib.as_array(getattr(obs, f))[:n] for f in ("tpz", "tplon", "tplat")])
    assert np.linalg.norm(synth._cart(*tp.T) - synth._cart(*ref["tp"].T), axis=1).max() < 1e-7
    i = int(np.argmax(ref["np"]))
    one = _obs(case.geom, 2)
    hip.formod_pencil(case.ctl, atm, one, i)
    hip.dropin_finalize()
    assert np.array_equal(np.ctypeslib.as_array(one.rad)[i, :2], rad[i])


@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_leaving_the_slice_at_the_first_point(hip, oracle, arrangement):
    """The two rays of test_scenes_cpu.test_leaving_the_slice_at_the_first_point (a slice 1 cm thick, seen from above:
    the LOS leaves it at its first point, which is then the whole LOS with ds = 0, unclipped) against the oracle."""
    case = common.limb_case()
    spec = [dict(time=0.0, lon=0.0, lat=0.0, n=2, z0=10.0, z1=10.00001), dict(time=1.0, lon=0.0, lat=0.0, n=30, z0=0.0, z1=60.0)]
    case.atm = synth.ragged_atmosphere(case.ctl, spec, base=case.atm)
    case.geom = np.array([[0.0, 700.0, 0.0, 0.0, 0.0, 0.0, 0.5], [0.0, 700.0, 0.0, 0.0, 9.9, 0.0, 0.0]])
    ref = oracle.formod_rays(case.ctl, case.atm, case.oracle_tables(oracle), case.geom)
    assert np.all(ref["np"] == 1)
    assert_parity(run(hip, case, arrangement), ref)
