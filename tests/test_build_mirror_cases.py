"""Which configurations reach the octant-mirror build kernel and which of its 72 compiled instances they run (no GPU): the planner
(bhw_describe_plan) against a rule restated in Python, and the probe window the GPU sweep rests on against the CPU oracle."""
import numpy as np
import pytest

import build_mirror_cases as C
import oracle_lib as O
from blackman_harris_win_amd import binding as B

DEAD_REASON = ("1 024-thread workgroups need a table of 2^24 entries, i.e. PW >= 26; z_shr == 0 needs PW <= W, so W >= 26 and the chain "
               "has at least 25 rotations: <21..24, *, 1024> cannot be reached")


def _walk(pws, precisions):
    """{(configuration, limit name): (instance, cell log)} by the planner, asserted equal to the restated rule on the whole grid."""
    seen = {}
    for c in C.grid(pws, precisions):
        rule = C.mirror_rule(*c)
        for mk in (C.bh7_params, C.probe_params):
            try:
                p = mk(*c)
            except B.BhwError:
                assert rule is None, ("the library refuses a configuration the rule sends to the mirror kernel", c)
                continue
            for name, limit, fmt in C.LIMITS:
                got = C.plan_instance(p, limit)
                want = (rule[0], fmt, rule[1]) if rule else None
                assert got == want, (c, name, mk.__name__, got, want)
                if got:
                    seen[(c, name)] = (got, rule[2])
    return seen


@pytest.fixture(scope="module")
def tested():
    return _walk(C.PW_TESTED, C.PRECISIONS)


def test_planner_and_restated_rule_agree_on_176_configurations(tested):
    cfgs = C.configurations()
    assert {c for c, _ in tested} == set(cfgs)
    assert len(cfgs) == 176
    per = {}
    for model, _, _, precision in cfgs:
        per[(model, precision)] = per.get((model, precision), 0) + 1
    assert per == {("hls", 1): 39, ("cpp", 1): 39, ("vhdl", 1): 39, ("vhdl", 2): 39, ("vhdl", 7): 20}


def test_pw_22_to_26_reach_60_instances_and_the_other_12_are_dead(tested):
    reached = {inst for inst, _ in tested.values()}
    assert len(reached) == 60
    assert C.ALL_INSTANCES - reached == C.DEAD_INSTANCES, DEAD_REASON
    # every instance the dispatch can reach at all is reached at PW <= 26: the longer windows (and the precisions in between) add none
    wide = _walk(range(22, 31), {"hls": (1,), "cpp": (1,), "vhdl": (1, 2, 3, 7)})
    assert {inst for inst, _ in wide.values()} == reached, DEAD_REASON


def test_every_cell_log_occurs_with_every_format(tested):
    for _, _, fmt in C.LIMITS:
        assert {d for (n, f, t), d in tested.values() if f == fmt and t == 256} == {7, 8, 9}
        assert {d for (n, f, t), d in tested.values() if f == fmt and t == 1024} == {9}        # PW 26: (50 - W) // 2 >= 9 at W <= 32


@pytest.mark.parametrize("model", sorted(C.MODELS))
@pytest.mark.parametrize("pw,w,precision", [(12, 16, 1), (14, 14, 1), (16, 24, 1), (14, 32, 1), (18, 22, 1), (16, 30, 2)])
def test_probe_window_is_minus_cosine_word_for_word(model, pw, w, precision):
    """What the GPU sweep rests on, proved on the reference alone: the oracle's window of probe_params is minus the oracle's cosine."""
    p = O.from_bhw(C.probe_params(model, pw, w, precision))
    window = O.generate_mt(p, 0, 1 << pw)
    _, cos = O.sincos_mt(p, 0, 1 << pw)
    assert np.array_equal(window, -cos)
