"""Atmosphere regridding (intpol_atm, IP = 1 / 2 / 3) at constructed edges, on the CPU: the oracle's restatement against
the extended-precision model of tests/edgecases.py (the library's intpol_atm needs a device; tests/test_intpol_edges_gpu.py
holds it to the oracle on the same cases).

Every case is written by hand (edgecases.intpol_cases): profiles of 2 to 8 levels with short decimal nodes, targets on
every node, at and beyond both ends of an axis, a descending axis, levels without pressure; tracks of 2 and 5 profiles of
unequal length with targets on a profile, at the tie of the two nearest and of the second and third nearest profile,
beyond both ends of the track, at 10 degrees of latitude from a profile and 2^-40 degrees further, with one and with no
profile in reach; point clouds with a candidate at dz == cz, one ulp inside, at dx2 == rm2, weights that sum to just
below and just above 1e-6, and a NaN in a point at a cut-off, which must not reach the result.  The model reports which
comparisons a target met with equality; the list is asserted for every target of every case.

Not reachable, hence without a case: r1 <= 0 with r0 > 0 (it needs dhmin0 - dhmin1 >= x^2 while dhmin0 <= dhmin1)."""
import numpy as np
import pytest
import edgecases as E


@pytest.mark.parametrize("name", E.intpol_case_names())
def test_oracle_regridding_at_constructed_edges(oracle, name):
    case, val, bnd, pexp, hits = E.intpol_ref(name)
    for j, (hit, expect) in enumerate(zip(hits, case["expect"])):
        assert hit == expect, (name, j, sorted(hit), sorted(expect))           # every target takes the branch it was built for
    dest = E.dest_atm(case["z"], case["lon"], case["lat"])
    assert oracle.intpol_atm(E.intpol_ctl(case["ip"], case["cx"], case["cz"]), dest, E.to_atm(case["src"])) == 0
    ratio = E.intpol_check(E.rows_of(dest), val, bnd)
    print("intpol %-50s oracle: worst error / allowed = %.3f" % (name, ratio))
    assert ratio <= 1


def test_the_cases_cover_the_edges():
    """every edge of the module docstring occurs in some case, at the sizes the kernel's 128-lane blocks call for"""
    cases = E.intpol_cases()
    seen = set().union(*[set().union(*c["expect"]) for c in cases])
    assert {"z == node", "z beyond the profile", "p <= 0: linear", "dhmin0 == 0", "r0 == 0", "dh == dhmin0", "dh == dhmin1",
            "dlat == 10", "one profile in reach", "no profile in reach", "r is NaN", "r0 < 0", "z beyond one of the two profiles",
            "dz == cz", "dz one ulp inside cz", "dx2 == rm2", "wsum just below 1e-6", "wsum just above 1e-6",
            "on a source point", "m = 0", "m = 1", "m = 2", "m = 3", "m = 4"} <= seen
    assert {len(c["z"]) for c in cases if c["ip"] == 1} == {1, 127, 128, 129}
    assert {len(c["src"]["z"]) for c in cases if c["ip"] == 1} == {2, 8}
    lengths = [tuple(E._profiles(c["src"])[1]) for c in cases if c["ip"] == 2]
    assert lengths == [(8, 2), (2, 8, 3, 8, 5)]
    assert all(len(c["src"]["z"]) <= 12 for c in cases if c["ip"] == 3)
    holes = next(c for c in cases if "p = 0" in c["name"])["src"]["rows"]
    assert (holes[0] == 0).sum() == 1 and (holes[3] == 0).sum() == 1
