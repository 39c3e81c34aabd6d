"""Call sequences on one long-lived model (helper of tests/test_sequences_gpu.py and tests/test_sequences_cpu.py).

A SCRIPT is a literal list of steps (tuples of names, numbers and dicts: it can be printed and pasted into a test).
`Runner.run` executes it on long-lived models and, after every step that computes something, compares the step's
outputs BIT FOR BIT (NaN-aware) with the same single call on a FRESH model: default knobs, the process-wide tuning
reset, the same arithmetic mode, the same atmosphere set once.  Bit equality is the derived tolerance: the suite
already proves that arrangement, chunking, ray order, lanes per ray, grouping and the compact layout do not change a
bit (test_pencil_gpu.py, test_parity_gpu.py, test_multi_gpu.py), so whatever a model carries from call to call must
not either.  Every distinct fresh answer is tied to the oracle on at most 300 sampled rays (assert_parity of
test_parity_gpu.py; tile and chunk boundaries are part of the sample).

Steps (first element = operation kind; the model meant is the current one, see "model"):

  ("model", name, family)               make `name` the current model, created on first use from FAMILIES[family]
  ("set_atm", atm_name)                 jur_model_set_atm with a NEW object built by atmosphere(family, atm_name)
  ("mutate_atm", level, dT)             edit one temperature of the object last passed IN PLACE, then set_atm it again
  ("formod_host", geom, opts)           opts: pinned (arrays from jur_host_alloc), mask (NaN / inf in rad_in), np (np_out)
  ("formod_device", geom, stream, opts) on the named torch stream; opts: sync=False leaves the call in flight -- its
                                        outputs are compared after the next step that waits
  ("contrib_host", geom) ("contrib_device", geom, stream) ("curtis_godson", geom) ("kernel", geom)
  ("fov_device", geom, stream)          jur_formod_device, then jur_fov_apply_device on its results
  ("knob", knob_name, *values)          see KNOBS
  ("nr0", entry)                        a call of zero rays: JUR_OK, nothing written
  ("invalid", which)                    see INVALID: arguments refused with JUR_EINVAL before any launch
  geom = (kind, n, seed): see geometry(); kind "overflow" holds rays that need more than NLOS points on the "tall"
  atmosphere -- a reported status (JUR_ENLOS, or the device status word) with the point counts clamped, not a fault.
"""
import ctypes as C
import hashlib
import pprint
import numpy as np
import common
from jurassic_hip import abi, synth

JUR_OK, JUR_EINVAL, JUR_ENLOS = 0, -1, -5

# call sizes that sit on the code's own constants: wavefront / tile (64), a block of 256 rays, the reference's package
# (NR = 1088), the fused kernel's limit (10 000), the staged-transfer limit of the host entry (JUR_SMALL_CALL = 65 536)
BOUNDARY_SIZES = (1, 63, 64, 65, 255, 257, 1088, 10000, 10001, 65536, 65537)

FAMILIES = {
    "std": lambda: common.retrieval_case(nu=common.CTM4_NU),       # 5 emitters x 4 channels, all four continua
    "hyd": lambda: common.retrieval_case(hydz=10.0),               # 5 emitters x 2 channels, hydrostatic step reads q_H2O
    "nadir": lambda: common.nadir_case(),                          # 1 emitter x 3 channels, WRITE_BBT, surface
}
ATMOSPHERES = ("base", "warm", "tall", "x4", "ragged")             # np: n, n, n, 4 n, 286 (synth.SCENES["ragged"])
GEOMETRIES = ("limb", "nadir", "mixed", "scan", "overflow", "beyond")
COMPUTE = ("formod_host", "formod_device", "contrib_host", "contrib_device", "curtis_godson", "kernel", "fov_device")

KNOBS = {
    "arithmetic": [(0,), (1,)],
    "pencil": [(0, 0), (10000, 0), (1 << 20, 4), (10000, 1), (1 << 20, 64)],
    "chunk_rays": [(64,), (4096,), (65536,), (1 << 21,)],
    "trace_multiple": [(1,), (4,), (64,)],
    "sort_rays": [(0,), (1,)],
    "compact_workspace": [(0,), (1,)],
    "workspace_budget": [(64 << 20,), (1 << 30,), (128 << 30,)],
    "tune_trace": [(0,), (1,), (4,)],
    "tune_combine": [(-1, 8, 1_000_000), (4, 8, 0), (0, 0, 0), (3, 2, 0), (6, -1, 0)],
    "reserve": [(64,), (1088,), (20000,), (70000,)],
}
INVALID = ("budget_small", "chunk_small", "arith_bad", "pencil_bad", "trace_mult_bad", "cg_nr0", "fov_n0", "atm_np1",
           "kernel_cols", "host_negative")
NR0_ENTRIES = ("formod_host", "formod_device", "contrib_host", "contrib_device")


# ---- inputs: functions of names and seeds alone --------------------------------------------------------------------
_cases = {}


def case_of(family):
    if family not in _cases:
        _cases[family] = FAMILIES[family]()
    return _cases[family]


def _copy_atm(a):
    out = abi.atm_t()
    C.memmove(C.byref(out), C.byref(a), C.sizeof(abi.atm_t))
    return out


def atmosphere(family, name):
    """A new atm_t: base (the family's profile), warm (same np, every temperature + 1.5 K), tall (same np, altitudes
    stretched by 1.08: low limb rays need more than NLOS points), x4 (four perturbed copies, time stamps 0 .. 3),
    ragged (synth.SCENES["ragged"]: five profiles of 2 .. 150 levels)."""
    case = case_of(family)
    if name == "base":
        return _copy_atm(case.atm)
    if name == "warm":
        a = _copy_atm(case.atm)
        np.ctypeslib.as_array(a.t)[:a.np] += 1.5
        return a
    if name == "tall":
        a = _copy_atm(case.atm)
        np.ctypeslib.as_array(a.z)[:a.np] *= 1.08
        return a
    if name == "x4":
        return synth.stack_profiles(case.atm, case.ctl, 4, seed=7)
    if name == "ragged":
        return synth.scene("ragged", case.ctl, case.atm, nrays=8, seed=3)[0]
    raise KeyError(name)


def atm_digest(atm):
    h = hashlib.sha1()
    n = atm.np
    h.update(str(n).encode())
    for f in ("time", "z", "lon", "lat", "p", "t"):
        h.update(np.ctypeslib.as_array(getattr(atm, f))[:n].tobytes())
    h.update(np.ctypeslib.as_array(atm.q)[:, :n].tobytes())
    h.update(np.ctypeslib.as_array(atm.k)[:, :n].tobytes())
    return h.hexdigest()


_scene_geom = {}


def geometry(family, atm_name, spec):
    """(n, 7) rays of spec = (kind, n, seed) for the atmosphere named.  limb / nadir / mixed: index-addressable rays
    (synth.limb_rays, nadir_rays) whose time stamps are the atmosphere's profiles; scan: one regular tangent-height scan
    (what the field-of-view convolution wants); overflow: a scan from 1.9 km up (its lowest rays need 398 .. 399 points
    on the 90 km atmospheres and more than NLOS on "tall"); beyond: limb rays of which every fifth carries a time stamp
    above the last profile (no line of sight: np = 0).  On "ragged" every kind is the scene's own rays (synth.scene:
    every profile, every azimuth, time stamps that match none), repeated to n."""
    kind, n, seed = spec
    if atm_name == "ragged":
        if family not in _scene_geom:
            case = case_of(family)
            _scene_geom[family] = synth.scene("ragged", case.ctl, case.atm, nrays=360, seed=3)[1]
        g = _scene_geom[family]
        return np.ascontiguousarray(np.roll(g, -seed % len(g), axis=0)[np.arange(n) % len(g)])
    npro = 4 if atm_name == "x4" else 1
    idx = np.arange(n, dtype=np.int64) + 7919 * seed
    if kind == "limb":
        g = synth.limb_rays(idx, nprofiles=npro)
    elif kind == "nadir":
        g = synth.nadir_rays(idx, nprofiles=npro)
    elif kind == "mixed":
        g = synth.limb_rays(idx, nprofiles=npro)
        g[1::2] = synth.nadir_rays(idx[1::2], nprofiles=npro)
    elif kind == "scan":
        g = synth.limb_geometry(n, scan=True, zmin=5.0, zmax=44.0)
    elif kind == "overflow":
        g = synth.limb_geometry(n, scan=True, zmin=1.9, zmax=1.9 + min(40.0, 0.05 * n))
        g[:, 0] = idx % npro
    elif kind == "beyond":
        g = synth.limb_rays(idx, nprofiles=npro)
        g[2::5, 0] = float(npro)
    else:
        raise KeyError(kind)
    return g


def rad_in_of(n, nd, mask):
    rad = np.zeros((n, nd))
    if mask:
        rad[0, nd - 1] = np.nan
        rad[n // 2, 0] = np.inf
        rad[n - 1, :] = np.nan
    return rad


# ---- comparison ------------------------------------------------------------------------------------------------------
def same_bits(got, want, what=""):
    """Every array of `want` equals that of `got` bit for bit (NaNs at the same places).  When the calls reported an
    overflow the rays that hit the clamp (np >= NLOS - 1) are left out: their content is not defined upstream either."""
    assert got["rc"] == want["rc"], (what, "rc", got["rc"], want["rc"], got.get("err"))
    assert got.get("status", 0) == want.get("status", 0), (what, "status")
    keep = None
    if (want["rc"] == JUR_ENLOS or want.get("status", 0)) and "np" in want:
        keep = want["np"] < abi.NLOS - 1
    for k, y in want.items():
        if not isinstance(y, np.ndarray) or (k == "np" and k not in got):       # (a host call without np_out)
            continue
        x = got[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape)
        if keep is not None and k not in ("k",):
            ax = 1 if k in ("rad_c", "tau_c") else 0
            x, y = np.compress(keep, x, axis=ax), np.compress(keep, y, axis=ax)
        if x.dtype.kind == "f":
            assert np.array_equal(np.isnan(x), np.isnan(y)), (what, k, "NaN mask")
            m = ~np.isnan(x)
            bad = x[m].view(np.uint64) != y[m].view(np.uint64)
            assert not bad.any(), (what, k, int(bad.sum()), "values differ", float(np.abs(x[m] - y[m]).max()))
        else:
            assert np.array_equal(x, y), (what, k)


def oracle_sample(n, seed, chunk=4096):
    """At most 300 ray indices of a call of n rays: both sides of every tile / block / package / path boundary that
    falls inside, the first chunk boundaries, the last ray, and seeded random ones."""
    edges = [0, 1, 62, 63, 64, 65, 127, 128, 254, 255, 256, 257, 1087, 1088, 9999, 10000, 10001, 65535, 65536, n - 1]
    edges += [c * chunk + d for c in range(1, 9) for d in (-1, 0)]
    idx = {i for i in edges if 0 <= i < n}
    if len(idx) < min(300, n):
        rng = np.random.default_rng(seed)
        idx |= set(int(i) for i in rng.integers(0, n, min(300, n) - len(idx)))
    return np.array(sorted(idx)[:300], dtype=np.int64)


# ---- single calls through the C ABI (status returned, not raised) ------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class Caller:
    """One entry each of include/jurassic_hip.h on a jurassic_hip.lib.Model; returns dict(rc=..., arrays...)."""

    def __init__(self, hip):
        self.hip, self.L = hip, hip.lib()
        self.streams = {}

    def err(self):
        return self.L.jur_last_error().decode()

    def stream(self, name):
        import torch
        if name == "default":
            return torch.cuda.current_stream()
        if name not in self.streams:
            self.streams[name] = torch.cuda.Stream()
        return self.streams[name]

    def formod_host(self, m, geom, rad_in, pinned=False, want_np=True):
        nr, nd = len(geom), m.nd
        b = self.hip.HostBuffers(nr, nd, pinned=pinned)
        b.set_geometry(geom)
        b.rad[...] = rad_in
        b.np[...] = -7
        dp = C.POINTER(C.c_double)
        garr = (dp * 7)(*[_dp(b.geom[k]) for k in range(7)])
        tarr = (dp * 3)(*[_dp(b.tp[k]) for k in range(3)])
        rc = self.L.jur_formod_host(m.h, nr, garr, _dp(b.rad), _dp(b.tau), tarr, _ip(b.np) if want_np else None)
        out = dict(rc=rc, err=self.err() if rc else "", rad=b.rad.copy(), tau=b.tau.copy(), tp=np.ascontiguousarray(b.tp.T))
        if want_np:
            out["np"] = b.np.copy()
        else:
            assert np.all(b.np == -7), "np_out was not given and was written"
        b.close()
        return out

    def contrib_host(self, m, geom, rad_in):
        g = np.ascontiguousarray(geom.T)
        nr, nd = len(geom), m.nd
        rad, tau, tp, npts = rad_in.copy(), np.zeros((nr, nd)), np.zeros((3, nr)), np.zeros(nr, dtype=np.int32)
        rad_c, tau_c = np.zeros((m.ng + 1, nr, nd)), np.zeros((m.ng + 1, nr, nd))
        dp = C.POINTER(C.c_double)
        garr = (dp * 7)(*[_dp(g[k]) for k in range(7)])
        tarr = (dp * 3)(*[_dp(tp[k]) for k in range(3)])
        rc = self.L.jur_formod_contrib_host(m.h, nr, garr, _dp(rad), _dp(tau), tarr, _ip(npts), _dp(rad_c), _dp(tau_c))
        return dict(rc=rc, err=self.err() if rc else "", rad=rad, tau=tau, tp=np.ascontiguousarray(tp.T), np=npts,
                    rad_c=rad_c, tau_c=tau_c)

    def curtis_godson(self, m, geom):
        g = np.ascontiguousarray(geom.T)
        nr = len(geom)
        out = [np.zeros((nr, max(m.ng, 1), abi.NLOS)) for _ in range(3)]
        npts = np.zeros(nr, dtype=np.int32)
        dp = C.POINTER(C.c_double)
        garr = (dp * 7)(*[_dp(g[k]) for k in range(7)])
        rc = self.L.jur_curtis_godson_host(m.h, nr, garr, _dp(out[0]), _dp(out[1]), _dp(out[2]), None, _ip(npts))
        return dict(rc=rc, err=self.err() if rc else "", cgp=out[0], cgt=out[1], cgu=out[2], np=npts)

    def kernel(self, m, atm, geom, nd, ncols=None):
        obs = common.obs_from_geom(geom, nd)
        obs.rad[min(5, len(geom) - 1)][nd - 1] = float("nan")            # a masked measurement drops its row
        n = self.L.jur_state_size(m.h, C.byref(atm)) if ncols is None else ncols
        rows = self.L.jur_measurement_size(m.h, C.byref(obs))
        k = np.full((rows, max(n, 1)), -7.0)
        rc = self.L.jur_kernel(m.h, C.byref(atm), C.byref(obs), _dp(k), rows, n)
        nr = len(geom)
        return dict(rc=rc, err=self.err() if rc else "", k=k, rad=np.ctypeslib.as_array(obs.rad)[:nr, :nd].copy(),
                    tau=np.ctypeslib.as_array(obs.tau)[:nr, :nd].copy(),
                    tp=np.stack([np.ctypeslib.as_array(getattr(obs, f))[:nr].copy() for f in ("tpz", "tplon", "tplat")], axis=1))

    def device_begin(self, m, geom, rad_in, stream, contrib=False):
        """Enqueue jur_formod_device / jur_formod_contrib_device on the named stream; -> pending call (no wait)."""
        import torch
        dev = torch.device("cuda", 0)
        nr, nd = len(geom), m.nd
        t = dict(geom=torch.from_numpy(np.ascontiguousarray(geom.T)).to(dev), rad=torch.from_numpy(rad_in.copy()).to(dev),
                 tau=torch.full((nr, nd), -7.0, dtype=torch.float64, device=dev),
                 tp=torch.full((3, nr), -7.0, dtype=torch.float64, device=dev),
                 np=torch.full((nr,), -7, dtype=torch.int32, device=dev), st=torch.zeros(1, dtype=torch.int32, device=dev))
        if contrib:
            t["rad_c"] = torch.full((m.ng + 1, nr, nd), -7.0, dtype=torch.float64, device=dev)
            t["tau_c"] = torch.full((m.ng + 1, nr, nd), -7.0, dtype=torch.float64, device=dev)
        s = self.stream(stream)
        s.wait_stream(torch.cuda.current_stream())                       # the inputs are ready; nothing else is waited for
        args = [t[k].data_ptr() for k in ("geom", "rad", "tau", "tp", "np", "st")]
        if contrib:
            rc = self.L.jur_formod_contrib_device(m.h, nr, *args, t["rad_c"].data_ptr(), t["tau_c"].data_ptr(), s.cuda_stream)
        else:
            rc = self.L.jur_formod_device(m.h, nr, *args, s.cuda_stream)
        return dict(rc=rc, err=self.err() if rc else "", t=t, s=s, contrib=contrib)

    def device_end(self, p):
        p["s"].synchronize()
        t = p["t"]
        out = dict(rc=p["rc"], err=p["err"], status=int(t["st"].item() != 0), rad=t["rad"].cpu().numpy(),
                   tau=t["tau"].cpu().numpy(), tp=np.ascontiguousarray(t["tp"].cpu().numpy().T), np=t["np"].cpu().numpy())
        if p["contrib"]:
            out["rad_c"], out["tau_c"] = t["rad_c"].cpu().numpy(), t["tau_c"].cpu().numpy()
        return out

    FOV_DZ = np.linspace(-1.5, 1.5, 21)
    FOV_W = np.exp(-0.5 * (np.linspace(-1.5, 1.5, 21) / 0.6) ** 2)

    def fov_device(self, m, geom, rad_in, stream, nshape=21):
        p = self.device_begin(m, geom, rad_in, stream)
        if p["rc"]:
            return self.device_end(p)
        t, s = p["t"], p["s"]
        rc = self.L.jur_fov_apply_device(m.h, len(geom), t["geom"][0].data_ptr(), t["geom"][4].data_ptr(), t["rad"].data_ptr(),
                                         t["tau"].data_ptr(), nshape, _dp(self.FOV_DZ), _dp(self.FOV_W), s.cuda_stream)
        p["rc"], p["err"] = rc, self.err() if rc else ""
        return self.device_end(p)


# ---- the runner --------------------------------------------------------------------------------------------------------
_fresh = {}       # (family, atm digest, entry, geom spec, arithmetic, mask) -> outputs of the single call on a fresh model
_oracle = {}      # (family, atm digest, geom spec, mask) -> (sample, oracle outputs)


class _Live:
    def __init__(self, family, model):
        self.family, self.model = family, model
        self.atm, self.atm_name, self.arith = None, None, 0


class Runner:
    def __init__(self, hip, oracle):
        self.hip, self.orc, self.call = hip, oracle, Caller(hip)
        self.models, self.cur, self.tune = {}, None, {"tune_trace": (0,), "tune_combine": (-1, 8, 1_000_000)}
        self.pending = []
        self.fresh_calls = 0

    # -- tuning that belongs to the process
    def _tune(self, name, values):
        (self.hip.tune_trace if name == "tune_trace" else self.hip.tune_combine)(*values)

    def _tune_default(self):
        self.hip.tune_trace(0)
        self.hip.tune_combine(-1, 8, 1_000_000)

    def _tune_restore(self):
        for name, values in self.tune.items():
            self._tune(name, values)

    def close(self):
        import torch
        torch.cuda.synchronize()
        for live in self.models.values():
            live.model.close()
        self.models.clear()
        self._tune_default()

    # -- one entry on one model
    def _single(self, model, live, entry, spec, opts, stream="default"):
        case = case_of(live.family)
        geom = geometry(live.family, live.atm_name, spec)
        rad_in = rad_in_of(len(geom), case.ctl.nd, opts.get("mask", False))
        c = self.call
        if entry == "formod_host":
            return c.formod_host(model, geom, rad_in, pinned=opts.get("pinned", False), want_np=opts.get("np", True))
        if entry == "formod_device":
            return c.device_end(c.device_begin(model, geom, rad_in, stream))
        if entry == "contrib_host":
            return c.contrib_host(model, geom, rad_in)
        if entry == "contrib_device":
            return c.device_end(c.device_begin(model, geom, rad_in, stream, contrib=True))
        if entry == "curtis_godson":
            return c.curtis_godson(model, geom)
        if entry == "kernel":
            return c.kernel(model, live.atm, geom, case.ctl.nd)
        if entry == "fov_device":
            return c.fov_device(model, geom, rad_in, stream)
        raise KeyError(entry)

    def fresh(self, live, entry, spec, opts):
        """The same single call on a fresh model: default knobs, process-wide tuning reset, the same arithmetic."""
        key = (live.family, atm_digest(live.atm), entry, spec, live.arith, bool(opts.get("mask", False)))
        if key not in _fresh:
            case = case_of(live.family)
            self._tune_default()
            m = self.hip.Model(case.ctl, case.lib_tables())
            m.set_arithmetic(live.arith)
            m.set_atm(_copy_atm(live.atm))
            shadow = _Live(live.family, m)
            shadow.atm, shadow.atm_name, shadow.arith = _copy_atm(live.atm), live.atm_name, live.arith
            out = self._single(m, shadow, entry, spec, dict(mask=opts.get("mask", False)))
            m.close()
            self._tune_restore()
            self.fresh_calls += 1
            self.tie_to_oracle(live, entry, spec, opts, out)
            _fresh[key] = out
        return _fresh[key]

    def tie_to_oracle(self, live, entry, spec, opts, out):
        """assert_parity (test_parity_gpu.py) of a fresh answer on at most 300 sampled rays.  Not for calls that
        reported an overflow (upstream and the oracle abort there) and not for the convolved radiances."""
        if out["rc"] != JUR_OK or out.get("status", 0) or entry == "fov_device":
            return
        from test_parity_gpu import assert_parity, RTOL
        case = case_of(live.family)
        mask = bool(opts.get("mask", False)) and entry != "kernel"
        okey = (live.family, atm_digest(live.atm), spec, mask, entry == "kernel")
        geom = geometry(live.family, live.atm_name, spec)
        if okey not in _oracle:
            sel = oracle_sample(len(geom), spec[2])
            rad_in = rad_in_of(len(geom), case.ctl.nd, mask)
            if entry == "kernel":
                rad_in[min(5, len(geom) - 1), case.ctl.nd - 1] = np.nan
            _oracle[okey] = (sel, self.orc.formod_rays(case.ctl, live.atm, case.oracle_tables(self.orc), geom[sel], rad_in=rad_in[sel]))
        sel, ref = _oracle[okey]
        if entry == "curtis_godson":
            assert np.array_equal(out["np"][sel], ref["np"])
            return
        got = {k: out[k][sel] for k in ("rad", "tau", "tp")}
        got["np"] = out["np"][sel] if "np" in out else ref["np"]
        assert_parity(got, ref, RTOL)

    def _flush(self):
        for live, entry, spec, opts, p, what in self.pending:
            same_bits(self.call.device_end(p), self.fresh(live, entry, spec, opts), what)
        self.pending = []

    # -- the script
    def run(self, script):
        i = -1
        try:
            for i, step in enumerate(script):
                self.step(step, "step %d %r" % (i, step))
            self._flush()
        except AssertionError as e:
            raise AssertionError("%s\nscript up to the failing step:\n%s" % (e, pprint.pformat(list(script[:i + 1]), width=120))) from e
        finally:
            self.pending = []
            self.close()

    def step(self, step, what):
        op, hip, L = step[0], self.hip, self.call.L
        if op == "model":
            name, family = step[1], step[2]
            if name not in self.models:
                case = case_of(family)
                self.models[name] = _Live(family, hip.Model(case.ctl, case.lib_tables()))
            self.cur = self.models[name]
            assert self.cur.family == family
            return
        live = self.cur
        m = live.model
        if op == "set_atm":
            live.atm, live.atm_name = atmosphere(live.family, step[1]), step[1]
            assert L.jur_model_set_atm(m.h, C.byref(live.atm)) == JUR_OK, (what, self.call.err())
        elif op == "mutate_atm":
            level = step[1] % live.atm.np
            live.atm.t[level] += step[2]                               # the SAME object, edited in place
            assert L.jur_model_set_atm(m.h, C.byref(live.atm)) == JUR_OK, (what, self.call.err())
        elif op == "knob":
            name, values = step[1], tuple(step[2:])
            if name in ("tune_trace", "tune_combine"):
                self.tune[name] = values
                self._tune(name, values)
            else:
                if name == "arithmetic":
                    live.arith = values[0]
                rc = getattr(L, "jur_model_reserve" if name == "reserve" else "jur_model_set_" + name)(m.h, *values)
                assert rc == JUR_OK, (what, self.call.err())
        elif op == "nr0":
            self.nr0(live, step[1], what)
        elif op == "invalid":
            self.invalid(live, step[1], what)
        elif op in COMPUTE:
            spec = tuple(step[1])
            opts = dict(step[-1]) if isinstance(step[-1], dict) else {}
            stream = step[2] if len(step) > 2 and isinstance(step[2], str) else "default"
            if op in ("formod_device", "contrib_device") and not opts.get("sync", True):
                case = case_of(live.family)
                geom = geometry(live.family, live.atm_name, spec)
                p = self.call.device_begin(m, geom, rad_in_of(len(geom), case.ctl.nd, opts.get("mask", False)), stream,
                                           contrib=(op == "contrib_device"))
                snap = _Live(live.family, None)
                snap.atm, snap.atm_name, snap.arith = _copy_atm(live.atm), live.atm_name, live.arith
                self.pending.append((snap, op, spec, opts, p, what))
                return
            got = self._single(m, live, op, spec, opts, stream)
            self._flush()                                              # calls left in flight before this one have ended too
            same_bits(got, self.fresh(live, op, spec, opts), what)
        else:
            raise KeyError(op)

    def nr0(self, live, entry, what):
        m, L = live.model, self.call.L
        one = np.full(8, -7.0)
        dp = C.POINTER(C.c_double)
        garr, tarr = (dp * 7)(*[_dp(one)] * 7), (dp * 3)(*[_dp(one)] * 3)
        if entry == "formod_host":
            rc = L.jur_formod_host(m.h, 0, garr, _dp(one), _dp(one), tarr, None)
        elif entry == "contrib_host":
            rc = L.jur_formod_contrib_host(m.h, 0, garr, _dp(one), _dp(one), tarr, None, _dp(one), _dp(one))
        elif entry == "formod_device":
            rc = L.jur_formod_device(m.h, 0, 0, 0, 0, 0, 0, 0, 0)
        elif entry == "contrib_device":
            rc = L.jur_formod_contrib_device(m.h, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        else:
            raise KeyError(entry)
        assert rc == JUR_OK and np.all(one == -7.0), (what, rc)

    def invalid(self, live, which, what):
        m, L = live.model, self.call.L
        one = np.full(8, -7.0)
        dp = C.POINTER(C.c_double)
        garr, tarr = (dp * 7)(*[_dp(one)] * 7), (dp * 3)(*[_dp(one)] * 3)
        if which == "budget_small":
            rc = L.jur_model_set_workspace_budget(m.h, 1)
        elif which == "chunk_small":
            rc = L.jur_model_set_chunk_rays(m.h, 1)
        elif which == "arith_bad":
            rc = L.jur_model_set_arithmetic(m.h, 7)
        elif which == "pencil_bad":
            rc = L.jur_model_set_pencil(m.h, -1, 0)
        elif which == "trace_mult_bad":
            rc = L.jur_model_set_trace_multiple(m.h, 0)
        elif which == "cg_nr0":
            rc = L.jur_curtis_godson_host(m.h, 0, garr, _dp(one), _dp(one), _dp(one), None, None)
        elif which == "fov_n0":
            rc = L.jur_fov_apply_device(m.h, 4, 0, 0, 0, 0, 0, _dp(one), _dp(one), 0)
        elif which == "atm_np1":
            a = _copy_atm(live.atm)
            a.np = 1
            rc = L.jur_model_set_atm(m.h, C.byref(a))
        elif which == "kernel_cols":
            case = case_of(live.family)
            rc = self.call.kernel(m, live.atm, geometry(live.family, live.atm_name, ("limb", 4, 0)), case.ctl.nd,
                                  ncols=L.jur_state_size(m.h, C.byref(live.atm)) + 1)["rc"]
        elif which == "host_negative":
            rc = L.jur_formod_host(m.h, -1, garr, _dp(one), _dp(one), tarr, None)
        else:
            raise KeyError(which)
        assert rc == JUR_EINVAL and np.all(one == -7.0), (what, rc)


# ---- seeded random scripts -----------------------------------------------------------------------------------------------
SEEDS = (11, 12, 13, 14, 15, 16)


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def generate(seed, nsteps=40):
    """A script from a seed: one model of the family seed % 3 picks (kernel steps: std and hyd only), mostly small
    calls, at most two above 65 536 rays, knobs (taken in turn, from a start the seed sets), atmospheres and refused calls
    in between."""
    rng = np.random.default_rng(seed)
    family = ("std", "hyd", "nadir")[seed % 3]
    script = [("model", "m", family), ("set_atm", "base")]
    atm, big, turn = "base", 0, 3 * seed
    entries = [e for e in COMPUTE if not (e == "kernel" and family == "nadir")]
    while len(script) < nsteps:
        r = rng.random()
        if r < 0.45:
            entry = _pick(rng, entries)
            u = rng.random()
            n = _pick(rng, BOUNDARY_SIZES[:7]) if u < 0.70 else _pick(rng, BOUNDARY_SIZES[7:9]) if u < 0.85 else _pick(rng, BOUNDARY_SIZES[9:])
            if entry in ("curtis_godson",):
                n = min(n, 1088)
            if entry == "kernel":
                n = min(n, 65)
            if entry == "fov_device":
                n = max(2, min(n, 10001))
            if entry == "contrib_host" or entry == "contrib_device":
                n = min(n, 65537 if family != "hyd" else 10001)
            if n > 65536:
                if big >= 2:
                    n = 65536
                else:
                    big += 1
            kind = "scan" if entry == "fov_device" else _pick(rng, ("limb", "limb", "nadir", "mixed", "beyond", "overflow"))
            if kind == "overflow":
                n = min(n, 1088)
            spec = (kind, int(n), int(rng.integers(0, 3)))
            if entry == "formod_host":
                script.append((entry, spec, dict(pinned=bool(rng.integers(0, 2)), mask=bool(rng.integers(0, 2)), np=bool(rng.integers(0, 2)))))
            elif entry in ("formod_device", "contrib_device", "fov_device"):
                script.append((entry, spec, _pick(rng, ("A", "B", "default"))))
            else:
                script.append((entry, spec))
        elif r < 0.73:
            name = sorted(KNOBS)[turn % len(KNOBS)]
            turn += 1
            script.append(("knob", name) + tuple(_pick(rng, KNOBS[name])))
        elif r < 0.85:
            if rng.random() < 0.35:
                script.append(("mutate_atm", int(rng.integers(0, 91)), float(_pick(rng, (0.25, -0.5, 1.0)))))
            else:
                atm = _pick(rng, ATMOSPHERES)
                script.append(("set_atm", atm))
        elif r < 0.93:
            script.append(("nr0", _pick(rng, NR0_ENTRIES)))
        else:
            which = _pick(rng, INVALID)
            if not (which == "kernel_cols" and family == "nadir"):
                script.append(("invalid", which))
    return script


# ---- what a set of scripts covers (tests/test_sequences_cpu.py) -------------------------------------------------------------
def call_sizes(script):
    return [step[1][1] for step in script if step[0] in COMPUTE]


def kind_counts(scripts):
    """How often each operation kind occurs: the compute entries, the two ways of set_atm, each knob, nr0, invalid, and
    calls that ask for an overflow."""
    n = {}
    for script in scripts:
        for step in script:
            keys = [step[0] if step[0] != "knob" else "knob:" + step[1]]
            if step[0] in COMPUTE and step[1][0] == "overflow":
                keys.append("overflow")
            for k in keys:
                n[k] = n.get(k, 0) + 1
    return n


def atm_points(family, name):
    return atmosphere(family, name).np


def may_fail(step, atm_name):
    """A step that ends in an error status: refused arguments, or overflow rays on the tall atmosphere."""
    return step[0] == "invalid" or (step[0] in COMPUTE and step[1][0] == "overflow" and atm_name == "tall")


def transitions(script):
    """-> set of the transitions a script makes: 'grow_shrink_grow' (call sizes a < b > c < d in a row), 'other_np'
    (set_atm to an atmosphere of another number of points), 'error_then_clean' (a step that ends in an error status
    followed by a compute call that does not)."""
    out, family, atm, np_now, failed = set(), None, None, None, False
    s = call_sizes(script)
    for a, b, c, d in zip(s, s[1:], s[2:], s[3:]):
        if a < b > c < d:
            out.add("grow_shrink_grow")
    for step in script:
        if step[0] == "model":
            family = step[2]
        elif step[0] == "set_atm":
            n = atm_points(family, step[1])
            if np_now is not None and n != np_now:
                out.add("other_np")
            atm, np_now = step[1], n
        if may_fail(step, atm):
            failed = True
        elif step[0] in COMPUTE:
            if failed:
                out.add("error_then_clean")
            failed = False
    return out


def validate(script):
    """Shape of a script: known operations, entries, knobs, atmospheres and geometry kinds; a model before anything."""
    assert script[0][0] == "model"
    for step in script:
        op = step[0]
        if op == "model":
            assert step[2] in FAMILIES
        elif op == "set_atm":
            assert step[1] in ATMOSPHERES
        elif op == "mutate_atm":
            assert isinstance(step[1], int) and isinstance(step[2], float)
        elif op == "knob":
            assert step[1] in KNOBS and len(step) > 2
        elif op == "nr0":
            assert step[1] in NR0_ENTRIES
        elif op == "invalid":
            assert step[1] in INVALID
        else:
            assert op in COMPUTE, op
            kind, n, seed = step[1]
            assert kind in GEOMETRIES and n >= 1 and seed >= 0
            assert n <= 1088 or op not in ("curtis_godson", "kernel"), step


# ---- fixed scripts: one per way a model carries state from call to call (jur_model.c) ------------------------------------
H = "formod_host"
FIXED = {
    # ensure_workspace: a held allocation serves smaller strides (use_rays, use_trace_rays, use_compact, d_eps_off and the
    # h_tile offset derived from ws_trace_rays carry over); the budget shrinks and grows again; 10 001 rays with chunks
    # of 4 096 and 257 rays with chunks of 64 are calls above the chunk size in use
    "workspace_larger_smaller_larger": [
        ("model", "m", "std"), ("set_atm", "x4"),
        (H, ("limb", 10001, 0), {}), ("knob", "chunk_rays", 4096), (H, ("limb", 10001, 0), {}), (H, ("mixed", 257, 1), {}),
        ("knob", "workspace_budget", 64 << 20), (H, ("limb", 65537, 0), {}), ("knob", "compact_workspace", 0),
        (H, ("mixed", 10001, 1), {}), ("knob", "workspace_budget", 128 << 30), ("knob", "chunk_rays", 1 << 21),
        (H, ("limb", 65536, 1), {}), ("knob", "compact_workspace", 1), ("knob", "trace_multiple", 4), ("knob", "chunk_rays", 64),
        ("knob", "pencil", 0, 0), (H, ("mixed", 257, 1), {}), (H, ("limb", 65, 0), {}), (H, ("limb", 63, 0), {}), (H, ("nadir", 1, 0), {}),
        ("knob", "sort_rays", 0), (H, ("limb", 1088, 0), {}), ("knob", "workspace_budget", 1 << 30), ("knob", "chunk_rays", 65536),
        ("formod_device", ("limb", 65537, 0), "A"), ("knob", "sort_rays", 1), ("knob", "trace_multiple", 64),
        ("formod_device", ("limb", 10001, 0), "B"), ("curtis_godson", ("limb", 255, 0)), (H, ("limb", 65537, 0), {})],
    # ensure_io grows d_io / h_io; the package threshold (65 536 / 65 537: staged image against transfers in place beside
    # the kernels), the fused kernel's (10 000 / 10 001: zero-copy against copy commands); pinned and pageable arrays
    "io_image_across_the_thresholds": [
        ("model", "m", "std"), ("set_atm", "base"),
        (H, ("limb", 64, 0), dict(pinned=True)), (H, ("limb", 65536, 0), {}), (H, ("limb", 65537, 0), dict(pinned=True)),
        (H, ("limb", 65537, 0), dict(mask=True)), (H, ("mixed", 65536, 1), dict(pinned=True, mask=True)),
        (H, ("limb", 10000, 0), {}), (H, ("limb", 10001, 0), dict(pinned=True, np=False)), (H, ("limb", 10000, 0), dict(pinned=True, mask=True)),
        (H, ("limb", 10001, 0), dict(mask=True)), (H, ("nadir", 1, 0), dict(np=False)),
        (H, ("mixed", 65537, 1), dict(mask=True, np=False)), (H, ("limb", 1088, 0), dict(pinned=True, np=False))],
    # jur_model_set_atm: atmospheres of 91, 4 x 91 and a synth.SCENES one alternating (atm_cap: smaller, larger, smaller);
    # the same np with other content; an equal atmosphere in a new object (the memcmp that skips the upload)
    "atmospheres_alternate": [
        ("model", "m", "std"), ("set_atm", "base"), (H, ("limb", 255, 0), {}), ("set_atm", "x4"), (H, ("limb", 1088, 0), {}),
        ("set_atm", "ragged"), (H, ("limb", 257, 0), {}), ("set_atm", "base"), (H, ("limb", 255, 0), {}), ("set_atm", "base"),
        ("formod_device", ("mixed", 10001, 0), "A"), ("set_atm", "warm"), (H, ("limb", 255, 0), {}), ("set_atm", "x4"),
        ("formod_device", ("mixed", 10001, 0), "A", dict(sync=False)), ("set_atm", "ragged"), ("curtis_godson", ("limb", 64, 0)),
        ("set_atm", "tall"), (H, ("nadir", 65, 0), {}), ("set_atm", "x4"), ("contrib_host", ("beyond", 1088, 1))],
    # the caller edits one temperature of the atm_t it passed and sets it again: the memcmp must see it
    "in_place_temperature_edit": [
        ("model", "m", "std"), ("set_atm", "base"), (H, ("limb", 65, 0), {}), ("mutate_atm", 30, 1.0), (H, ("limb", 65, 0), {}),
        ("mutate_atm", 0, -0.5), ("formod_device", ("limb", 10001, 0), "A"), ("mutate_atm", 90, 0.25), ("kernel", ("limb", 63, 0)),
        ("mutate_atm", 45, 0.25), (H, ("limb", 65, 0), {}),
        ("model", "h", "hyd"), ("set_atm", "base"), ("contrib_host", ("limb", 64, 0)), ("mutate_atm", 12, 1.0), ("contrib_host", ("limb", 64, 0))],
    # the status word after a call that overflowed NLOS, then a clean call, on every entry ("tall": scans from 1.9 km up
    # need more than 400 points, nadir rays do not)
    "overflow_then_clean_on_every_entry": [
        ("model", "m", "std"), ("set_atm", "tall"),
        (H, ("overflow", 64, 0), {}), (H, ("nadir", 64, 0), {}), (H, ("overflow", 10001, 0), {}), (H, ("nadir", 10001, 0), {}),
        ("formod_device", ("overflow", 255, 0), "A"), ("formod_device", ("nadir", 255, 0), "A"),
        ("formod_device", ("overflow", 10001, 0), "B"), ("formod_device", ("nadir", 10001, 0), "B"),
        ("contrib_host", ("overflow", 65, 0)), ("contrib_host", ("nadir", 65, 0)),
        ("contrib_device", ("overflow", 65, 0), "A"), ("contrib_device", ("nadir", 65, 0), "A"),
        ("curtis_godson", ("overflow", 63, 0)), ("curtis_godson", ("nadir", 63, 0)),
        ("kernel", ("overflow", 8, 0)), ("kernel", ("nadir", 8, 0)),
        ("fov_device", ("scan", 64, 0), "A"), ("set_atm", "base"), ("fov_device", ("scan", 64, 0), "A"), (H, ("overflow", 64, 0), {})],
    # jur_kernel stacks n + 1 atmospheres on the device and puts the caller's back: the next call needs no set_atm (rays
    # whose time stamp lies above the profile find nothing in it -- and would find a perturbed copy in a stack)
    "kernel_then_formod_host_without_set_atm": [
        ("model", "m", "std"), ("set_atm", "base"), ("kernel", ("limb", 64, 0)), (H, ("beyond", 257, 0), {}),
        ("kernel", ("limb", 1, 0)), ("formod_device", ("beyond", 10001, 0), "A"), ("set_atm", "x4"), ("kernel", ("limb", 8, 0)),
        ("curtis_godson", ("beyond", 65, 0)),
        ("model", "h", "hyd"), ("set_atm", "base"), ("kernel", ("limb", 65, 0)), ("contrib_host", ("limb", 63, 0)), (H, ("beyond", 64, 0), {})],
    # ... after an error return too: JUR_ENLOS from jur_kernel must not leave the stack behind (the contribution entry
    # with HYDZ >= 0 insists on an atmosphere that jur_model_set_atm put there)
    "kernel_overflow_then_formod_host": [
        ("model", "m", "std"), ("set_atm", "tall"), ("kernel", ("overflow", 8, 0)), (H, ("beyond", 257, 0), {}),
        ("kernel", ("overflow", 8, 0)), ("curtis_godson", ("nadir", 64, 0)), ("kernel", ("overflow", 8, 0)), ("set_atm", "tall"),
        (H, ("nadir", 65, 0), {}),
        ("model", "h", "hyd"), ("set_atm", "tall"), ("kernel", ("overflow", 8, 0)), ("contrib_host", ("nadir", 64, 0)),
        ("kernel", ("overflow", 8, 0)), (H, ("beyond", 64, 0), {})],
    # contributions with HYDZ >= 0 and H2O trace ng edited atmospheres stacked on the device, then put the caller's back
    "contrib_hydrostatic_then_plain_call": [
        ("model", "h", "hyd"), ("set_atm", "base"), ("contrib_host", ("limb", 255, 0)), (H, ("beyond", 255, 0), {}),
        ("contrib_device", ("limb", 65, 0), "A"), ("formod_device", ("beyond", 65, 0), "B"), ("curtis_godson", ("limb", 63, 0)),
        ("set_atm", "x4"), ("contrib_host", ("mixed", 1088, 0)), (H, ("mixed", 1088, 0), {}), ("contrib_host", ("limb", 10001, 0)),
        ("set_atm", "tall"), ("contrib_host", ("overflow", 64, 0)), (H, ("nadir", 64, 0), {}), ("contrib_host", ("nadir", 64, 0))],
    # jur_model_set_arithmetic between calls, through the fused and the batched kernels and the Jacobian
    "fast_exact_fast": [
        ("model", "m", "std"), ("set_atm", "base"), (H, ("limb", 1088, 0), {}), ("formod_device", ("limb", 10001, 0), "A"),
        ("knob", "arithmetic", 1), (H, ("limb", 1088, 0), {}), ("formod_device", ("limb", 10001, 0), "A"), ("kernel", ("limb", 64, 0)),
        ("contrib_host", ("limb", 255, 0)), ("knob", "arithmetic", 0), (H, ("limb", 1088, 0), {}),
        ("formod_device", ("limb", 10001, 0), "A"), ("kernel", ("limb", 64, 0)), ("contrib_host", ("limb", 255, 0))],
    # jur_model_set_pencil, chunking, trace multiple, sort and compact settings between calls of one size
    "switches_between_calls": [
        ("model", "m", "std"), ("set_atm", "x4"), (H, ("mixed", 10000, 0), {}), ("knob", "pencil", 1 << 20, 4), (H, ("mixed", 10001, 0), {}),
        ("knob", "pencil", 10000, 1), (H, ("mixed", 1088, 0), {}), ("knob", "pencil", 0, 0), (H, ("mixed", 1088, 0), {}),
        ("knob", "chunk_rays", 64), ("knob", "trace_multiple", 64), (H, ("mixed", 10000, 0), {}), ("knob", "sort_rays", 0),
        (H, ("mixed", 10000, 0), {}), ("knob", "compact_workspace", 0), ("knob", "workspace_budget", 64 << 20), (H, ("mixed", 10001, 0), {}),
        ("knob", "reserve", 70000), ("knob", "pencil", 1 << 20, 64), (H, ("mixed", 255, 0), {}), ("knob", "sort_rays", 1),
        ("knob", "pencil", 10000, 0), ("knob", "reserve", 1088), ("formod_device", ("mixed", 1088, 0), "A")],
    # the process-wide jur_tune_trace / jur_tune_combine (and the LDS-limit bits behind them) with two models of other
    # ng / nd alive at once
    "two_models_interleaved_while_tuning_changes": [
        ("model", "a", "std"), ("set_atm", "x4"), ("model", "b", "nadir"), ("set_atm", "base"),
        ("knob", "tune_combine", 4, 8, 0), ("model", "a", "std"), (H, ("limb", 10001, 0), {}), ("model", "b", "nadir"), (H, ("nadir", 10001, 0), {}),
        ("knob", "tune_trace", 4), ("model", "a", "std"), ("formod_device", ("limb", 10001, 0), "A", dict(sync=False)),
        ("model", "b", "nadir"), ("formod_device", ("nadir", 10001, 0), "B"), ("knob", "tune_trace", 1), ("knob", "tune_combine", 3, 2, 0),
        ("knob", "pencil", 0, 0), (H, ("mixed", 1088, 0), {}), ("model", "a", "std"), (H, ("limb", 65537, 0), {}),
        ("knob", "tune_combine", 6, -1, 0), ("knob", "tune_trace", 0), ("model", "b", "nadir"), ("contrib_host", ("nadir", 257, 0)),
        ("model", "a", "std"), ("contrib_host", ("limb", 257, 0)), ("knob", "tune_combine", 0, 0, 0), (H, ("limb", 10001, 0), {}),
        ("model", "b", "nadir"), (H, ("nadir", 10001, 0), {})],
    # grow-only scratch: the sort buffers, d_kq / h_kq (Jacobian), d_fov, d_ctb -- larger, smaller, larger
    "grow_only_scratch": [
        ("model", "m", "std"), ("set_atm", "base"), ("knob", "pencil", 0, 0),
        (H, ("limb", 257, 0), {}), (H, ("limb", 10001, 0), {}), (H, ("limb", 65, 0), {}), (H, ("mixed", 10001, 1), {}),
        ("kernel", ("limb", 1, 0)), ("kernel", ("limb", 65, 0)), ("kernel", ("limb", 63, 0)), ("kernel", ("limb", 65, 0)),
        ("fov_device", ("scan", 255, 0), "A"), ("fov_device", ("scan", 10001, 0), "A"), ("fov_device", ("scan", 65, 0), "B"),
        ("fov_device", ("scan", 10000, 0), "default"),
        ("contrib_host", ("limb", 64, 0)), ("contrib_host", ("limb", 10001, 0)), ("contrib_host", ("limb", 63, 0)),
        ("contrib_host", ("mixed", 65537, 0))],
    # calls that are refused before any launch, and calls of no rays, leave the model as it was
    "refused_and_empty_calls": [
        ("model", "m", "std"), ("set_atm", "x4"), (H, ("limb", 255, 0), {})] +
        [s for w in INVALID for s in (("invalid", w), (H, ("limb", 255, 0), {}))] +
        [s for e in NR0_ENTRIES for s in (("nr0", e), ("formod_device", ("limb", 10001, 0), "A"))],
    # stream ordering: 200 000 rays on stream A, at once 20 000 other rays on stream B into other buffers (the smaller call
    # fits the workspace the first one holds: nothing reallocates), then the host entry, jur_curtis_godson_host and
    # jur_kernel on the model's own stream while a device-entry call is still running
    "calls_on_two_streams_then_the_host_entry": [
        ("model", "m", "std"), ("set_atm", "x4"),
        ("formod_device", ("limb", 200000, 0), "A", dict(sync=False)), ("formod_device", ("mixed", 20000, 1), "B", dict(sync=False)),
        (H, ("limb", 10001, 2), {}),
        ("formod_device", ("limb", 200000, 0), "B", dict(sync=False)), ("curtis_godson", ("mixed", 255, 1)),
        ("formod_device", ("limb", 200000, 0), "A", dict(sync=False)), ("kernel", ("limb", 64, 0)),
        ("formod_device", ("limb", 200000, 0), "A", dict(sync=False)), ("contrib_host", ("mixed", 10001, 1)),
        ("formod_device", ("limb", 200000, 0), "B", dict(sync=False)), ("set_atm", "base"), (H, ("limb", 10001, 2), {})],
}
