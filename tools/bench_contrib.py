#!/usr/bin/env python3
"""One contribution call (jur_formod_contrib_device: the forward model plus the spectrum of every emitter and of the
extinction alone) against the ng + 2 separate jur_formod_device calls it replaces (the total, then every edited
atmosphere), all arrays resident on the device, after warm-up.  Prints one JSON document.

  python3 tools/bench_contrib.py [--shape refspec|limb_1e5|both] [--reps N] [--out FILE]

refspec:  66 limb rays at 3 .. 68 km, 100 channels from 1050 cm^-1, 30 emitters (the reference's refspec example)
limb_1e5: 1e5 limb rays, 4 channels (all four continua), 5 emitters, 64 profiles (bench.py's limb atmosphere)

The separate calls are timed one by one (synchronised), without the atmosphere uploads between them; the wall time of
the whole sequence with the uploads is reported too.  The kernel shares come from a third, event-timed contribution
call."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import common
from jurassic_hip import abi, lib, synth

REFSPEC_EMITTERS = ["C2H2", "C2H6", "CCl4", "CH4", "ClO", "ClONO2", "CO", "CO2", "COF2", "F11", "F12", "F14", "F22", "H2O",
                    "H2O2", "HCN", "HNO3", "HNO4", "HOCl", "N2", "N2O", "N2O5", "NH3", "NO", "NO2", "O2", "O3", "OCS", "SF6",
                    "SO2"]


def refspec_case(tmpdir):
    rows = np.loadtxt(os.path.join(common.GOLD, "limb", "atm.tab"), comments="#")      # time z lon lat p T q[5] k
    wide = np.hstack([rows[:, :6], np.tile(rows[:, 6:11], (1, 6)), rows[:, 11:12] + 1e-5])
    path = os.path.join(tmpdir, "atm30.tab")
    np.savetxt(path, wide, fmt="%.17g")
    return common.Case(REFSPEC_EMITTERS, [1050.0 + i for i in range(100)], path, common.golden_geometry("limb"),
                       table_kw=dict(nlev=12, ntemp=5))


def edited_atm(case, v):
    a = abi.atm_t()
    C.memmove(C.byref(a), C.byref(case.atm), C.sizeof(abi.atm_t))
    q, k = np.ctypeslib.as_array(a.q), np.ctypeslib.as_array(a.k)
    for g in range(case.ctl.ng):
        if g != v:
            q[g, :] = 0.0
    if v < case.ctl.ng:
        k[:, :] = 0.0
    return a


def measure(case, reps):
    import torch
    dev = torch.device("cuda:0")
    nr, nd, ng = len(case.geom), case.ctl.nd, case.ctl.ng
    m = lib.Model(case.ctl, case.lib_tables())
    m.set_atm(case.atm)
    geom = torch.tensor(np.ascontiguousarray(case.geom.T), device=dev)
    rad = torch.zeros((nr, nd), dtype=torch.float64, device=dev)
    tau, tp = torch.zeros_like(rad), torch.zeros((3, nr), dtype=torch.float64, device=dev)
    rad_c = torch.zeros((ng + 1, nr, nd), dtype=torch.float64, device=dev)
    tau_c = torch.zeros_like(rad_c)
    a = (geom.data_ptr(), rad.data_ptr(), tau.data_ptr(), tp.data_ptr())

    def contrib():
        rad.zero_()
        m.formod_contrib_device(nr, *a, rad_c.data_ptr(), tau_c.data_ptr())

    def one():
        rad.zero_()
        m.formod_device(nr, *a)

    atms = [case.atm] + [edited_atm(case, v) for v in range(ng + 1)]
    for _ in range(2):                                  # warm-up: workspace, sort buffers, code objects
        contrib()
        for at in atms:
            m.set_atm(at)
            one()
        m.set_atm(case.atm)
    torch.cuda.synchronize()
    t_contrib, t_sep, t_sep_wall = [], [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        contrib()
        torch.cuda.synchronize()
        t_contrib.append(time.perf_counter() - t0)
        tot, w0 = 0.0, time.perf_counter()
        for at in atms:
            m.set_atm(at)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one()
            torch.cuda.synchronize()
            tot += time.perf_counter() - t0
        t_sep_wall.append(time.perf_counter() - w0)
        t_sep.append(tot)
        m.set_atm(case.atm)
    m.enable_timing(True)
    contrib()
    torch.cuda.synchronize()
    k = m.kernel_ms()
    c = m.contrib_ms()
    m.enable_timing(False)
    m.close()
    kern = dict(trace_ms=k["trace_ms"], ega_ms=k["ega_ms"], combine_ms=k["combine_ms"], contrib_ms=c["contrib_ms"],
                launches=k["ega_launches"])
    ksum = kern["trace_ms"] + kern["ega_ms"] + kern["combine_ms"] + kern["contrib_ms"]
    med = lambda x: float(np.median(x)) * 1e3
    return dict(rays=nr, channels=nd, emitters=ng, spectra=ng + 2, reps=reps,
                contrib_call_ms=med(t_contrib), separate_calls_ms=med(t_sep), separate_calls_with_uploads_ms=med(t_sep_wall),
                speedup=med(t_sep) / med(t_contrib), speedup_with_uploads=med(t_sep_wall) / med(t_contrib),
                kernels_event_timed=kern, contrib_kernel_share=kern["contrib_ms"] / ksum if ksum > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["refspec", "limb_1e5", "both"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import tempfile
    import torch
    torch.cuda.is_available()
    res = dict(tool="tools/bench_contrib.py", device=torch.cuda.get_device_name(0), shapes={})
    with tempfile.TemporaryDirectory() as tmp:
        if args.shape in ("refspec", "both"):
            res["shapes"]["refspec"] = measure(refspec_case(tmp), args.reps)
        if args.shape in ("limb_1e5", "both"):
            case = common.limb_case(geom=synth.limb_geometry(100000, seed=1, nprofiles=64), nu=common.CTM4_NU, nprofiles=64)
            res["shapes"]["limb_1e5"] = measure(case, args.reps)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
