"""``sings_amd.density.HybridDensitySchedule`` against the event lists the reference's own ``_adjust_density`` produced
(tests/golden/density_schedule_golden.json, written by tests/golden/gen_density_schedule_golden.py): event for event, with the final
``densify_interval``; ``decides_at`` against ``actions`` at every iteration; the switch points of ``l2_keys`` and ``sh_up``; a
``state_dict`` taken in the middle of a run; the refusal of an iteration out of order."""
import json
import os

import pytest

from sings_amd.density import HybridDensitySchedule

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "density_schedule_golden.json")) as f:
        return json.load(f)


def _schedule(entry, **kw):
    cfg = {k: v for k, v in entry["config"].items() if k != "steps"}
    return HybridDensitySchedule(**cfg, **kw), entry["config"]["steps"]


def _events(sch, t0, t1):
    return [[t, mode] for t in range(t0, t1) for mode in sch.actions(t)]


@pytest.mark.parametrize("name", ["human_male", "defaults", "compressed"])
def test_actions_reproduce_the_references_events(golden, name):
    sch, steps = _schedule(golden[name])
    assert _events(sch, 0, steps) == golden[name]["events"]
    assert sch.densify_interval == golden[name]["densify_interval"]


def test_the_goldens_hold_what_the_rule_is_known_for(golden):
    """The quirks, read off the recorded lists themselves (not off the code under test)."""
    c, d = golden["compressed"], golden["defaults"]
    assert c["events"] == [[3, "prune"], [5, "densify"], [7, "prune"], [8, "densify"], [11, "prune"], [11, "densify"], [13, "densify"]]
    assert c["densify_interval"] == 4
    assert d["events"][:3] == [[1999, "prune"], [1999, "densify"], [3999, "prune"]] and d["densify_interval"] == 2001
    assert golden["human_male"]["densify_interval"] == 1500 and len(golden["human_male"]["events"]) == 7


@pytest.mark.parametrize("name", ["human_male", "defaults", "compressed"])
def test_decides_at_agrees_with_actions_at_every_iteration(golden, name):
    sch, steps = _schedule(golden[name])
    for t in range(steps):
        before = sch.state_dict()
        decides = sch.decides_at(t)
        assert sch.state_dict() == before                        # (asking changes nothing)
        assert decides == bool(sch.actions(t)), t


def test_l2_keys_switch_when_both_windows_have_closed(golden):
    sch, _ = _schedule(golden["compressed"])                     # prune until 12, densify until 14
    assert [t for t in range(20) if "opacity" in sch.l2_keys(t)] == list(range(14, 20))
    assert sch.l2_keys(13) == ("xyz_offsets", "scales") and sch.l2_keys(14) == ("xyz_offsets", "scales", "opacity")
    male, _ = _schedule(golden["human_male"])                    # prune until 6000, densify until 10000
    assert "opacity" not in male.l2_keys(9999) and "opacity" in male.l2_keys(10000)
    swapped = HybridDensitySchedule(0, 10000, 5, 0, 6000, 5)     # (the later of the two, whichever it is)
    assert "opacity" not in swapped.l2_keys(9999) and "opacity" in swapped.l2_keys(10000)


def test_sh_up(golden):
    sch, _ = _schedule(golden["compressed"])
    assert [t for t in range(3001) if sch.sh_up(t)] == [1000, 2000, 3000]
    five, _ = _schedule(golden["compressed"], sh_up_every=5)
    assert [t for t in range(16) if five.sh_up(t)] == [5, 10, 15]


@pytest.mark.parametrize("cut", [4, 11, 12])
def test_a_state_dict_taken_mid_run_continues_identically(golden, cut):
    entry = golden["compressed"]
    first, steps = _schedule(entry)
    head = _events(first, 0, cut)
    sd = json.loads(json.dumps(first.state_dict()))              # (plain data: it survives a file)
    second, _ = _schedule(entry)
    second.load_state_dict(sd)
    assert second.densify_interval == first.densify_interval
    assert head + _events(second, cut, steps) == entry["events"]
    assert second.densify_interval == entry["densify_interval"]
    with pytest.raises(ValueError):
        second.actions(cut - 1)                                  # (the loaded state knows where the run was)


def test_iterations_out_of_order_are_refused(golden):
    sch, _ = _schedule(golden["compressed"])
    sch.actions(0); sch.actions(1); sch.actions(5)
    for t in (5, 4, 0):
        with pytest.raises(ValueError, match="once per iteration"):
            sch.actions(t)
    assert sch.actions(6) == ()


def test_thresholds_reach_the_two_calls(golden):
    sch, _ = _schedule(golden["compressed"], prune_opacity_threshold=0.3, prune_scale_threshold=0.0005, prune_max_n_gs_once=5000,
                       min_n_gaussians=100000, densify_grad_threshold=0.001, densify_scale_threshold=0.005,
                       densify_render_size_threshold=20, max_n_gaussians=200000)
    assert sch.prune_kwargs() == dict(opacity_threshold=0.3, scale_threshold=0.0005, prune_max_n_gs_once=5000, min_n_gs=100000)
    assert sch.densify_kwargs() == dict(grad_threshold=0.001, scale_threshold=0.005, max_screen_size=20, max_n_gs=200000)
