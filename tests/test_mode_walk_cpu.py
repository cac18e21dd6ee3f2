"""The table of states of tests/test_mode_walk_gpu.py stays complete: every ShadeMode (csrc/pt_types.h) and every FormUnit
(csrc/pt_forms.h) is put in effect by a state of common.WALK_STATES, the pair sequence holds every ordered pair of states, and the
family sequence gives every state a neighbour of another bounce-word layout on both sides. A new mode or unit fails here until it
gets a state. No GPU."""
import os
import re

import pytest

import common

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thu-acg-f2024-path-tracer_amd", "csrc")


def _enumerators(header, enum):
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"\benum\s+" + enum + r"\s*\{([^}]*)\}", text)
    assert m, f"{header}: enum {enum} not found"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip().split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert names and all(re.fullmatch(r"[A-Z_0-9]+", n) for n in names), names
    return names


def test_every_shade_mode_has_a_state():
    modes = [n for n in _enumerators("pt_types.h", "ShadeMode") if n != "N_SHADE_MODES"]      # (their number, not a mode)
    assert len(modes) >= 7
    assert set(modes) == set(common.WALK_MODE_STATE), "a ShadeMode without a state (or a mapping to a mode that is gone)"
    assert all(s in common.WALK_STATES for s in common.WALK_MODE_STATE.values())


def test_every_form_unit_has_a_state():
    units = _enumerators("pt_forms.h", "FormUnit")
    assert len(units) >= 10
    assert set(units) == set(common.WALK_UNIT_STATE), "a FormUnit without a state (or a mapping to a unit that is gone)"
    assert all(s in common.WALK_STATES for s in common.WALK_UNIT_STATE.values())


def test_states_families_and_sampler_exceptions():
    in_families = [s for f in common.WALK_FAMILIES for s in f]
    assert sorted(in_families) == sorted(common.WALK_STATES), "every state is in exactly one bounce-word family"
    # every state is the image of a mode or a unit, but for INT2: the second way into the INT mode (a glass interior, behind a rebuild)
    named = set(common.WALK_MODE_STATE.values()) | set(common.WALK_UNIT_STATE.values())
    assert set(common.WALK_STATES) - named == {"INT2"}
    # the states left out of the sampler axis, each with its reason: pt_forms.h has a QMC form for every mode, MOT and PLT, so there are none
    assert len(common.WALK_NO_QMC) == 0
    assert all(s in common.WALK_STATES and isinstance(why, str) and why for s, why in common.WALK_NO_QMC.items())
    # ... as long as shade_form_exists gives the default variant's shapes every (list, qmc, motion, mode): its rule, whitespace aside
    text = "".join(open(os.path.join(CSRC, "pt_forms.h")).read().split())
    rule = "s.variant == 22 || s.variant == 32 || s.variant == 42 || !(list || qmc || motion || mode != MODE_PLAIN)"
    assert "".join(rule.split()) in text, "shade_form_exists changed: check which states still have forms for the Sobol sampler (common.WALK_NO_QMC)"
    assert common.walk_states(True) == list(common.WALK_STATES)
    assert common.walk_states(False) == [s for s in common.WALK_STATES if s != "LSE"]


@pytest.mark.parametrize("lights", [True, False])
def test_pair_sequence_holds_every_ordered_pair(lights):
    states = common.walk_states(lights)
    seq = common.walk_pair_circuit(states)
    n = len(states)
    assert len(seq) == n * (n - 1) + 1 and seq[0] == seq[-1] == "PLAIN"
    pairs = list(zip(seq, seq[1:]))
    assert len(set(pairs)) == len(pairs) and all(a != b for a, b in pairs)
    assert set(pairs) == {(a, b) for a in states for b in states if a != b}
    assert seq == common.walk_pair_circuit(states), "deterministic"


@pytest.mark.parametrize("lights", [True, False])
def test_family_sequence_has_cross_family_neighbours(lights):
    states = common.walk_states(lights)
    seq = common.walk_family_sequence(states)
    assert seq[0] == seq[-1] and sorted(seq[:-1]) == sorted(states)
    fam = common.walk_family
    assert all(fam(a) != fam(b) for a, b in zip(seq, seq[1:]))
    for s in states:      # (the first state's predecessor is at the walk's closing visit)
        visits = [i for i, x in enumerate(seq) if x == s]
        assert any(i > 0 and fam(seq[i - 1]) != fam(s) for i in visits), f"{s} has no predecessor of another family"
        assert any(i + 1 < len(seq) and fam(seq[i + 1]) != fam(s) for i in visits), f"{s} has no successor of another family"
