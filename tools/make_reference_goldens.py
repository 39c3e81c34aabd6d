#!/usr/bin/env python3
"""Writes tests/golden/reference_runs/: what the reference's own CPU forward model (oracle/_ref/libjurassic_ref.so,
`make -C oracle ref`) returns on every case of tests/refcases.py -- per formod case one float64 .npy
(rad | tau | tpz tplon tplat side by side, one row per ray), per Jacobian case the matrix ((131, 69); (197, 69) for the three channels of
jacobian_nd3_bbt) in two halves of its rows -- and
manifest.json with one line per case: name, shape, sha256 over the case's inputs (refcases.input_hash).

Needs the reference tree (JUR_REFERENCE) to have been present at build time; the results are data the reference's
program wrote, its sources are not read by this tool.     usage: tools/make_reference_goldens.py [case ...]"""
import json
import os
import sys
import tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jurassic-gpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import refcases as R  # noqa: E402
from oracle import orc, ref  # noqa: E402


def main(names):
    assert ref.available(), "oracle/_ref/libjurassic_ref.so is missing: make -C oracle ref"
    os.makedirs(R.STORE, exist_ok=True)
    path = os.path.join(R.STORE, "manifest.json")
    entries = {}
    if names and os.path.exists(path):
        entries = R.manifest()
    for name in names or list(R.FORMOD) + list(R.JACOBIANS):
        with tempfile.TemporaryDirectory() as d:
            if name in R.JACOBIANS:
                case, obs = R.jacobian_case(name)
                case.write_files(d)
                rad_in = np.ctypeslib.as_array(obs.rad)[:obs.nr, :case.ctl.nd].copy()
                m, n = int(np.isfinite(rad_in).sum()), orc.state_size(case.ctl, case.atm)
                arr, _ = ref.kernel(case.ctl, case.atm, obs, m, n)
            else:
                case, rad_in = R.FORMOD[name]()
                case.write_files(d)
                arr = R.pack(R.run_reference(ref, case, rad_in))
            digest = R.input_hash(case, d, rad_in)
        files = R.store(name, arr)
        entries[name] = dict(case=name, shape=list(arr.shape), sha256=digest)
        print("%-28s %-10s %s" % (name, arr.shape, " ".join(f + ".npy" for f in files)), flush=True)
    with open(path, "w") as fh:
        fh.write('{"cases": [\n' + ",\n".join(json.dumps(e, sort_keys=True) for e in entries.values()) + "\n]}\n")


if __name__ == "__main__":
    main(sys.argv[1:])
