"""The Jacobian reused between the iterations of Model.retrieve_scene (jur_model_set_kernel_recomp), the part that needs
no GPU: the new entries are exported with the header's signatures, the Python wrappers refuse wrongly shaped blocks, the
map from the rays that remain to the blocks a Jacobian iteration left (jur_scene_recomp_offsets) agrees with a search, and
the forward-only passes of a reuse iteration fit what jur_scene_pass_reserve reserves.

The seeded scenes and the caps are those of tests/test_scene_passes_cpu.py."""
import ctypes as C
import itertools
import os
import re
import numpy as np
import pytest
import common
from jurassic_hip import lib
from test_scene_passes_cpu import CASES, remaining, rowptr

NEW = ("jur_model_set_kernel_recomp", "jur_model_kernel_recomp", "jur_gradient_scene_host", "jur_scene_recomp_offsets")


def kind(param):
    """pointer, long or int: what a parameter of a prototype is to the caller"""
    if "*" in param or "[" in param:
        return "pointer"
    return "long" if re.search(r"\blong\b", param) else "int"


def kind_of_ctype(t):
    if t in (C.c_long, C.c_size_t):
        return "long"
    if t is C.c_int:
        return "int"
    return "pointer"


def test_the_new_entries_are_exported_with_the_headers_signatures():
    L = lib.lib()
    hdr = open(os.path.join(common.ROOT, "include", "jurassic_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        found = re.search(r"\b(int|long)\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert found, "%s is not declared in jurassic_hip.h" % name
        params = [p.strip() for p in found.group(2).split(",")]
        args = getattr(L, name).argtypes
        assert args is not None and [kind(p) for p in params] == [kind_of_ctype(t) for t in args], (name, params, args)
        restype = getattr(L, name).restype
        assert (restype is C.c_long) == (found.group(1) == "long"), name


def test_the_map_refuses_what_it_cannot_answer():
    with pytest.raises(lib.JurassicError, match=r"error %d: jur_scene_recomp_offsets: slice 1 of ray 1 is active but was not" % lib.EINVAL):
        lib.scene_recomp_offsets([0, 2, 5], [0, 1], [0, 1], [0, 0], 2)
    with pytest.raises(lib.JurassicError, match=r"error %d: jur_scene_recomp_offsets: bad arguments" % lib.EINVAL):
        lib.scene_recomp_offsets([0, 2, 5], [0, 1], [0, 0], [0, 0], 0)
    with pytest.raises(ValueError, match=r"sid must be \(2,\)"):
        lib.scene_recomp_offsets([0, 2, 5], [0, 1, 1], [0, 0], [0, 0], 2)
    assert list(lib.scene_recomp_offsets([0], [], [], [], 3)) == []
    assert list(lib.scene_recomp_offsets([0, 2, 2, 5], [0, -1, 1], [0, 0], [0, 0], 3)) == [0, 6]   # (a ray without elements is in no pass)


def searched(w, sid, then, now, nd):
    """the first double of the block of every ray that is active now, by a search: a Jacobian iteration wrote the blocks
    of the rays that were active then one after the other"""
    written = [r for r in range(len(w)) if sid[r] >= 0 and then[sid[r]] == 0]
    start = {}
    at = 0
    for r in written:
        start[r] = at
        at += int(w[r]) * nd
    return [start[r] for r in range(len(w)) if sid[r] >= 0 and now[sid[r]] == 0]


@pytest.mark.parametrize("make,seed", CASES, ids=["%s-%d" % (m.__name__, s) for m, s in CASES])
def test_the_map_agrees_with_a_search(make, seed):
    """for every set of slices that had ended at the Jacobian iteration and every larger set that has ended now"""
    w, sid, _ = make(seed)
    rp = rowptr(w)
    ns = int(sid.max()) + 1
    live = sorted(set(sid[sid >= 0].tolist()))
    checked = 0
    for k in range(len(live)):
        for ended_then in itertools.combinations(live, k):
            then = np.isin(np.arange(ns), ended_then).astype(np.int32)      # (1: converged, any state but 0 has ended)
            rest = [s for s in live if s not in ended_then]
            for j in range(len(rest)):
                for more in itertools.combinations(rest, j):
                    now = then.copy()
                    now[list(more)] = 2
                    for nd in (1, 3):
                        got = lib.scene_recomp_offsets(rp, sid, then, now, nd)
                        assert list(got) == searched(w, sid, then, now, nd), (seed, ended_then, more, nd)
                    checked += 1
    assert checked >= 3


@pytest.mark.parametrize("make,seed", CASES, ids=["%s-%d" % (m.__name__, s) for m, s in CASES])
def test_forward_only_passes_fit_the_reserve(make, seed):
    """A reuse iteration cuts jur_trial_passes(n, 1, cap) on the rays that remain; the loop reserves
    jur_scene_pass_reserve(nr, rowptr, cap, nlam).  Every such pass, for every cap, every nlam and every set of ended
    slices (none among them), has no more slots than that."""
    w, sid, time = make(seed)
    rp = rowptr(w)
    keeps = [keep for _, keep in remaining(sid)] + [sid >= 0, np.ones(len(w), dtype=bool)]
    for cap in range(1, int(rp[-1]) + len(w) + 2):
        for ntrial in (1, 3):
            slots, _ = lib.scene_pass_reserve(rp, cap, ntrial, time)
            for keep in keeps:
                need = lib.trial_passes(int(keep.sum()), 1, cap, None if time is None else time[keep])[1]
                assert need <= slots, (seed, cap, ntrial, need, slots)


def test_the_wrappers_refuse_wrongly_shaped_blocks():
    """(before the library is called: no GPU is needed to be refused)"""
    case = common.limb_case()
    model = lib.Model.__new__(lib.Model)                                 # the wrapper's checks read ctl and nd alone
    model.ctl, model.nd, model.h = case.ctl, case.ctl.nd, None
    geom = case.geom[:4]
    nr, nd = len(geom), case.ctl.nd
    lay = lib.scene_layout(case.ctl, case.atm, geom[:, 0])
    nk = int(lay["rowptr"][-1]) * nd
    y, weight = np.zeros((nr, nd)), np.ones((nr, nd))
    for bad in [np.zeros(nk + 1), np.zeros((nk, 1))] + ([np.zeros(nk - 1)] if nk else []):
        with pytest.raises(ValueError, match=r"k must be the flat blocks of these rays"):
            model.gradient_scene(case.atm, geom, y, weight, bad)
    with pytest.raises(ValueError, match=r"y and weight must be"):
        model.gradient_scene(case.atm, geom, y[:, :1], weight, np.zeros(nk))
