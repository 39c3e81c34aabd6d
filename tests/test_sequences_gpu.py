"""What a model carries from one call to the next (jur_model.c: workspace, I/O image, atmosphere, status word, switches,
grow-only scratch, the event that orders calls on different streams) must not show in any result: scripts of calls on
long-lived models, every step held BIT FOR BIT to the same single call on a fresh model with default knobs, and every
distinct fresh answer to the oracle (tests/sequences.py has the vocabulary, the runner and the scripts).

Fixed scripts, one per hazard (sequences.FIXED, each with the state it is after written above it); seeded random
scripts (sequences.SEEDS; tests/test_sequences_cpu.py holds them to their coverage condition without a GPU).  A failing
step prints the script up to it as a literal list: paste it into FIXED to keep it.

Replaying a captured graph after a step that may reallocate is not among the scripts: that is an invalid address by
the caller's doing (include/jurassic_hip.h: jur_model_reserve).

Wall time on an MI355X: not measured yet (DESIGN.md section 2 has the rule: a quarter of the rest of the GPU suite at
most; over that, random seeds go, fixed scripts stay)."""
import pytest
import sequences as sq

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


@pytest.fixture(scope="module")
def hip():
    from jurassic_hip import lib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return lib


@pytest.mark.parametrize("name", sorted(sq.FIXED))
def test_fixed_script(hip, oracle, name):
    sq.Runner(hip, oracle).run(sq.FIXED[name])


@pytest.mark.parametrize("seed", sq.SEEDS)
def test_random_script(hip, oracle, seed):
    sq.Runner(hip, oracle).run(sq.generate(seed))


def test_a_stale_answer_is_caught_and_printed(hip, oracle):
    """The runner's own check: when the model holds another atmosphere than the one the fresh model is given (here: the
    runner's record of it is swapped behind the model's back), the step fails and the message carries the script."""
    script = [("model", "m", "std"), ("set_atm", "base"), ("nr0", "formod_host"), ("formod_host", ("limb", 65, 0), {})]

    class Swapped(sq.Runner):
        def step(self, step, what):
            if step[0] == "nr0":
                self.cur.atm = sq.atmosphere("std", "warm")            # the model still holds "base"
            return super().step(step, what)

    with pytest.raises(AssertionError, match=r"values differ(.|\n)*script up to the failing step:\n\[\('model', 'm', 'std'\)"):
        Swapped(hip, oracle).run(script)
    sq.Runner(hip, oracle).run(script)
