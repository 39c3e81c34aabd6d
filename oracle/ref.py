"""The reference's own CPU forward model (oracle/_ref/libjurassic_ref.so, built by `make -C oracle ref` from the
reference tree where it lies) -- TEST INFRASTRUCTURE, CPU only.

The reference keeps its tables, its continuum gas indices and its field-of-view shape in process-wide statics that
are initialised once (get_tbl, formod_CPU, formod_fov), and the table set alone is 8.8 GB of virtual memory at ND = 100,
NG = 30.  So every configuration runs in a fresh child process: `python -m oracle.ref <workdir>`, inputs and outputs as
.npy files in the work directory, the reference's stdout and stderr in <workdir>/ref.log.  The child imports numpy and
ctypes only -- never torch, never the HIP library -- and the parent starts it as an ordinary subprocess.

    formod(ctl, atm, obs)        -> obs (a copy) after the reference's formod()
    kernel(ctl, atm, obs, m, n)  -> (k (m, n), obs) after the reference's kernel()
    formod_fov(ctl, obs)         -> obs after formod_fov() (ctl.fov names the shape file)
    intpol_atm(ctl, dest, src)   -> dest after intpol_atm()
    hydrostatic(ctl, atm)        -> atm after hydrostatic()

ctl.tblbase must name table and filter files on disk (Case.write_files); USEGPU is forced to 0.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "_ref", "libjurassic_ref.so")
DEFAULT_TREE = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "jurassic-gpu_amd"))
from jurassic_hip import abi  # noqa: E402


def tree():
    return os.environ.get("JUR_REFERENCE", DEFAULT_TREE)


def available():
    """The library has been built (here, or on the box the tree was copied from)."""
    return os.path.exists(SO)


def required():
    """The reference tree is present: the recipe can build the library, so a missing library is a failure there."""
    return os.path.exists(os.path.join(tree(), "src", "jurassic.c"))


class GslMatrix(C.Structure):
    """GSL's gsl_matrix layout, as jurassic_hip.lib.GslMatrix and oracle/gsl_standin/gsl/gsl_blas.h have it."""
    _fields_ = [("size1", C.c_size_t), ("size2", C.c_size_t), ("tda", C.c_size_t), ("data", C.POINTER(C.c_double)),
                ("block", C.c_void_p), ("owner", C.c_int)]


_TYPES = {"ctl": abi.ctl_t, "atm": abi.atm_t, "obs": abi.obs_t, "atm2": abi.atm_t}


def _dump(workdir, name, struct):
    np.save(os.path.join(workdir, name + ".npy"), np.frombuffer(bytes(struct), dtype=np.uint8))


def _load(workdir, name, cls):
    raw = np.load(os.path.join(workdir, name + ".npy")).tobytes()
    assert len(raw) == C.sizeof(cls), (name, len(raw), C.sizeof(cls))
    return cls.from_buffer_copy(raw)


def _run(call, structs, args=(), workdir=None, threads=None):
    if not available():
        raise RuntimeError("oracle/_ref/libjurassic_ref.so is missing: run `make -C oracle ref` with the reference tree")
    own = workdir is None
    tmp = tempfile.TemporaryDirectory() if own else None
    wd = tmp.name if own else workdir
    try:
        for name, s in structs.items():
            _dump(wd, name, s)
        env = dict(os.environ, JUR_ND=str(abi.ND), JUR_NG=str(abi.NG))
        if threads:
            env["OMP_NUM_THREADS"] = str(threads)
        with open(os.path.join(wd, "ref.log"), "w") as log:
            r = subprocess.run([sys.executable, "-m", "oracle.ref", wd, call] + [str(a) for a in args], cwd=ROOT, env=env,
                               stdout=log, stderr=subprocess.STDOUT, timeout=1800)
        if r.returncode != 0:
            tail = open(os.path.join(wd, "ref.log")).read()[-2000:]
            raise RuntimeError("reference %s() ended with status %d:\n%s" % (call, r.returncode, tail))
        out = {name: _load(wd, name + "_out", _TYPES[name]) for name in structs if name != "ctl"}
        if call == "kernel":
            out["k"] = np.load(os.path.join(wd, "k_out.npy"))
        return out
    finally:
        if tmp:
            tmp.cleanup()


def _cpu(ctl):
    c = abi.ctl_t.from_buffer_copy(bytes(ctl))
    c.useGPU = 0
    return c


def formod(ctl, atm, obs, workdir=None):
    return _run("formod", dict(ctl=_cpu(ctl), atm=atm, obs=obs), workdir=workdir)["obs"]


def kernel(ctl, atm, obs, m, n, workdir=None):
    out = _run("kernel", dict(ctl=_cpu(ctl), atm=atm, obs=obs), (m, n), workdir=workdir)
    return out["k"], out["obs"]


def formod_fov(ctl, obs, workdir=None):
    return _run("formod_fov", dict(ctl=_cpu(ctl), obs=obs), workdir=workdir)["obs"]


def intpol_atm(ctl, dest, src, workdir=None):
    """-> (dest after the call, or None where the reference aborted; the log's tail)."""
    try:
        return _run("intpol_atm", dict(ctl=_cpu(ctl), atm=dest, atm2=src), workdir=workdir)["atm"], ""
    except RuntimeError as e:
        return None, str(e)


def hydrostatic(ctl, atm, workdir=None):
    return _run("hydrostatic", dict(ctl=_cpu(ctl), atm=atm), workdir=workdir)["atm"]


def arrays(obs, nd):
    """obs_t -> dict(rad (nr, nd), tau (nr, nd), tp (nr, 3)) as Model.formod_host and orc.formod_rays return them."""
    n = obs.nr
    a = {k: np.ctypeslib.as_array(getattr(obs, k))[:n, :nd].copy() for k in ("rad", "tau")}
    a["tp"] = np.stack([np.ctypeslib.as_array(getattr(obs, k))[:n] for k in ("tpz", "tplon", "tplat")], axis=1).copy()
    return a


def _child(wd, call, args):
    L = C.CDLL(SO)
    s = {name: _load(wd, name, cls) for name, cls in _TYPES.items() if os.path.exists(os.path.join(wd, name + ".npy"))}
    ctl = s["ctl"]
    vp = C.c_void_p
    if call == "formod":
        L.formod.argtypes = [vp, vp, vp]
        L.formod.restype = None
        L.formod(C.byref(ctl), C.byref(s["atm"]), C.byref(s["obs"]))
    elif call == "kernel":
        m, n = int(args[0]), int(args[1])
        store = np.zeros((m, n))
        mat = GslMatrix(m, n, n, store.ctypes.data_as(C.POINTER(C.c_double)), None, 0)
        L.kernel.argtypes = [vp, vp, vp, vp]
        L.kernel.restype = None
        L.kernel(C.byref(ctl), C.byref(s["atm"]), C.byref(s["obs"]), C.byref(mat))
        np.save(os.path.join(wd, "k_out.npy"), store)
    elif call == "formod_fov":
        L.formod_fov.argtypes = [vp, vp]
        L.formod_fov.restype = None
        L.formod_fov(C.byref(ctl), C.byref(s["obs"]))
    elif call == "intpol_atm":
        L.intpol_atm.argtypes = [vp, vp, vp]
        L.intpol_atm.restype = None
        L.intpol_atm(C.byref(ctl), C.byref(s["atm"]), C.byref(s["atm2"]))
    elif call == "hydrostatic":
        L.hydrostatic.argtypes = [vp, vp]
        L.hydrostatic.restype = None
        L.hydrostatic(C.byref(ctl), C.byref(s["atm"]))
    else:
        raise SystemExit("unknown call " + call)
    for name in s:
        if name != "ctl":
            _dump(wd, name + "_out", s[name])


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3:])
