"""The restated gym oracle equals the VERBATIM reference module step by step (float64), for the shipped config variants and
the feature switches, with the reference's own MT19937 consumption order -- against the reference's outputs recorded in
tests/golden/ref_traces_mt19937.npz (tests/golden/make_reference_traces.py: the same seed, actions and auto-resets)."""
import copy
import json
import os

import numpy as np
import pytest

import configs
from golden import make_reference_traces as mrt
from oracle.gym_restated import FixedWingOracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cmp(leaves, schema, values, path):
    """Worst |ours - recorded| over one event; the key paths, shapes and NaN positions must agree."""
    got = {p: v for p, v in leaves}
    want = {p: s for p, s in schema}
    assert set(got) == set(want), (path, sorted(set(got) ^ set(want)))
    worst, off = 0.0, 0
    for p, shape in schema:
        if shape is None:
            assert got[p] is None, (path, p, "a dict in the reference")
            continue
        a = got[p]
        assert a is not None and list(a.shape) == shape, (path, p, None if a is None else a.shape, shape)
        b = values[off:off + a.size].reshape(a.shape)
        off += a.size
        assert np.array_equal(np.isnan(a), np.isnan(b)), (path, p, a, b)
        if a.size:
            worst = max(worst, float(np.max(np.abs(np.where(np.isnan(a), 0, a - b)))))
    return worst, off


CASES = mrt.CASES


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restated_gym_equals_verbatim_reference(case):
    name, kind, ckw, skw = case
    with np.load(os.path.join(GOLDEN, "ref_traces_mt19937.npz"), allow_pickle=False) as z:
        layout = json.loads(str(z[name + ":layout"]))
        values = z[name + ":values"]
    assert layout["seed"] == mrt.SEED and layout["steps"] == mrt.STEPS
    events = iter(layout["events"])
    pos = [0]

    def check(kind_, leaves, done=False, termination=None, t=None):
        ev_kind, schema_id, ev_done, ev_term = next(events)
        assert ev_kind == kind_, (t, ev_kind, kind_)
        assert done == ev_done and termination == ev_term, (t, done, ev_done, termination, ev_term)
        w, n = _cmp(leaves, layout["schemas"][schema_id], values[pos[0]:], (kind_, t))
        pos[0] += n
        return w

    env = FixedWingOracle(configs.reference_like(kind), config_kw=copy.deepcopy(ckw), sim_config_kw=copy.deepcopy(skw))
    env.seed(mrt.SEED)
    worst = check("reset", mrt.event_leaves("reset", env.reset()))
    episodes = 0
    for t, a in enumerate(mrt.actions()):
        o, r, d, i = env.step(a.copy())
        worst = max(worst, check("step", mrt.event_leaves("step", o, r, i), bool(d), i.get("termination"), t))
        if d:
            episodes += 1
            worst = max(worst, check("reset", mrt.event_leaves("reset", env.reset()), t=t))
    assert next(events, None) is None and pos[0] == values.size   # every recorded event replayed
    assert worst < 1e-9, worst


# ---- the presets against the configuration FILES the reference ships ------------------------------------------------------
# keys a preset may carry / lack without changing what the environment computes, each with the reason it is inert
INERT = {
    "mlp": {"+": {"action.scale_high": "read only when action.scale_space is true (fixed_wing.py:349-354); the mlp file sets it false",
                  "action.scale_low": "as scale_high"}, "-": {}},
    "cnn": {"+": {}, "-": {"action.bounds_outside_cost": "never read by fixed_wing.py (grep: no occurrence)"}},
}
SHIPPED = mrt.SHIPPED   # (kind -> the file's path in the reference; the files themselves: tests/golden/ref_shipped_configs.json)


def _flat(d, prefix=""):
    out = {}
    if isinstance(d, dict):
        for k, v in d.items():
            out.update(_flat(v, prefix + ("." if prefix else "") + str(k)))
    elif isinstance(d, list):
        for i, v in enumerate(d):
            out.update(_flat(v, prefix + "[{}]".format(i)))
    else:
        out[prefix] = d
    return out


@pytest.mark.parametrize("kind", sorted(SHIPPED))
def test_preset_equals_the_shipped_configuration_file(kind):
    """presets.preset(kind) -- what the kernels are frozen for and what every test calls 'the reference's configuration' -- is
    the file the reference ships, key by key and value by value, modulo the stated inert keys."""
    from gym_fixed_wing import presets
    with open(os.path.join(GOLDEN, "ref_shipped_configs.json")) as f:
        recorded = json.load(f)
    assert recorded["configs"][kind]["file"] == SHIPPED[kind]
    shipped = _flat(recorded["configs"][kind]["config"])
    ours = _flat({k: v for k, v in presets.preset(kind).items() if k != "_comment"})
    extra = {k: v for k, v in ours.items() if k not in shipped}
    missing = {k: v for k, v in shipped.items() if k not in ours}
    differ = {k: (ours[k], shipped[k]) for k in ours if k in shipped and ours[k] != shipped[k]}
    allowed = INERT.get(kind, {"+": {}, "-": {}})
    assert set(extra) == set(allowed["+"]), ("keys only the preset has", extra)
    assert set(missing) == set(allowed["-"]), ("keys only the shipped file has", missing)
    assert not differ, differ
    # the inert keys really are: the reference module never reads `bounds_outside_cost`
    if kind == "cnn":
        assert recorded["module_mentions"]["bounds_outside_cost"] is False
