"""What the committed scripts of tests/sequences.py cover, checked without a GPU: the seeded random scripts
(sequences.SEEDS) must use every operation kind at least 5 times and every boundary call size at least twice, and make
each of the transitions grow / shrink / grow, another np, error then clean call; the fixed scripts are well formed and
reach every boundary size.  If a seed set misses the condition, the seeds change, not the condition."""
import sequences as sq

KINDS = (list(sq.COMPUTE) + ["set_atm", "mutate_atm", "nr0", "invalid", "overflow"] + ["knob:" + k for k in sorted(sq.KNOBS)])


def scripts():
    return [sq.generate(seed) for seed in sq.SEEDS]


def test_generated_scripts_are_reproducible_and_well_formed():
    for seed, script in zip(sq.SEEDS, scripts()):
        assert script == sq.generate(seed)
        sq.validate(script)
        sizes = sq.call_sizes(script)
        assert sum(n > 65536 for n in sizes) <= 2, (seed, sizes)
        assert sum(n <= 1088 for n in sizes) * 2 > len(sizes), (seed, "most steps are small")
        assert repr(eval(repr(script))) == repr(script)                  # a literal list: prints and pastes


def test_every_operation_kind_occurs_five_times():
    n = sq.kind_counts(scripts())
    assert {k: n.get(k, 0) for k in KINDS if n.get(k, 0) < 5} == {}


def test_every_boundary_size_occurs_twice():
    sizes = [n for script in scripts() for n in sq.call_sizes(script)]
    assert {n: sizes.count(n) for n in sq.BOUNDARY_SIZES if sizes.count(n) < 2} == {}


def test_every_transition_occurs():
    seen = set()
    for script in scripts():
        seen |= sq.transitions(script)
    assert seen >= {"grow_shrink_grow", "other_np", "error_then_clean"}, seen


def test_fixed_scripts_are_well_formed_and_reach_every_boundary_size():
    sizes = set()
    for name, script in sq.FIXED.items():
        sq.validate(script)
        sizes |= set(sq.call_sizes(script))
    assert sizes >= set(sq.BOUNDARY_SIZES), sorted(set(sq.BOUNDARY_SIZES) - sizes)
    assert any(n > 65537 for n in sizes)
