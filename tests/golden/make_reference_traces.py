#!/usr/bin/env python3
"""Generates the fixtures of tests/test_oracle_vs_reference.py -- BUILD CONTAINER ONLY (needs the reference checkout that
tests/golden/_ref_harness.py imports).

    python tests/golden/make_reference_traces.py

  ref_traces_mt19937.npz   for every case of the test: what the VERBATIM reference module returns from reset() / step() under
                           env.seed(3) (its own MT19937 consumption order, auto-reset at every episode end) for the test's
                           seeded action sequence -- observations, rewards, done flags, termination reasons and the info dicts,
                           float64.  Per case two entries: `<case>:values` (every number, in event order) and `<case>:layout`
                           (JSON: the key paths / shapes of each event and its done flag / termination reason)
  ref_shipped_configs.json the configuration files the reference ships (data), parsed, and whether the reference module's
                           source mentions the keys the presets treat as inert

Nothing of the reference's code travels: a fixture holds recorded outputs and configuration data only."""
import copy
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _ref_harness  # noqa: E402
import configs  # noqa: E402

TRACES = os.path.join(HERE, "ref_traces_mt19937.npz")
SHIPPED_CONFIGS = os.path.join(HERE, "ref_shipped_configs.json")

# (tests/test_oracle_vs_reference.py: the cases, the seed, the number of steps and the action sequence)
CASES = [c for c in configs.CASES if c[0] not in ("spec_c3",)] + configs.ORACLE_ONLY_CASES
SEED = 3
STEPS = 260
SHIPPED = {"default": "fixed_wing_config.json", "dev": "fixed_wing_config_dev.json", "examples": "examples/fixed_wing_config.json",
           "mlp": "examples/models/mlp_controller/fixed_wing_config.json", "cnn": "examples/models/cnn_controller/fixed_wing_config.json"}
INERT_KEYS = ("bounds_outside_cost",)


def actions(steps=STEPS):
    """The action of every step: a random walk that holds its value 70 % of the time."""
    rng = np.random.default_rng(1)
    a = rng.uniform(-1, 1, 3)
    out = []
    for _ in range(steps):
        if rng.uniform() < 0.3:
            a = np.clip(a + rng.normal(0, 0.4, 3), -1.8, 1.8)
        out.append(a.copy())
    return out


def flatten(x, path, out):
    """(key path, float64 array) leaves of nested dicts; a dict node is listed with shape None, so that an empty dict or a
    missing key still shows in the layout."""
    if isinstance(x, dict):
        out.append((path, None))
        for k in x:
            flatten(x[k], path + "/" + str(k), out)
    else:
        out.append((path, np.asarray(x, dtype=np.float64)))
    return out


def event_leaves(kind, obs, reward=None, info=None):
    """The values the test compares for one reset() or step() return."""
    if kind == "reset":
        return flatten(obs, "reset", [])
    leaves = flatten(obs, "obs", [])
    leaves += flatten(reward, "reward", [])
    return leaves + flatten({k: v for k, v in info.items() if k != "termination"}, "info", [])


def record(ref, case, workdir):
    name, kind, ckw, skw = case
    cfg = configs.reference_like(kind)
    path = os.path.join(workdir, "cfg_{}.json".format(name))
    with open(path, "w") as f:
        json.dump(cfg, f)
    env = ref.FixedWingAircraft(path, config_kw=copy.deepcopy(ckw), sim_config_kw=copy.deepcopy(skw))
    env.seed(SEED)
    schemas, events, values = [], [], []

    def add(kind_, leaves, done=False, termination=None):
        schema = [[p, None if v is None else list(v.shape)] for p, v in leaves]
        if schema not in schemas:
            schemas.append(schema)
        events.append([kind_, schemas.index(schema), bool(done), termination])
        values.extend(v.ravel() for _, v in leaves if v is not None)

    add("reset", event_leaves("reset", env.reset()))
    for a in actions():
        o, r, d, i = env.step(a.copy())
        add("step", event_leaves("step", o, r, i), d, i.get("termination"))
        if d:
            add("reset", event_leaves("reset", env.reset()))
    layout = {"case": name, "seed": SEED, "steps": STEPS, "schemas": schemas, "events": events}
    return layout, np.concatenate(values) if values else np.zeros(0)


def main():
    ref = _ref_harness.load_reference()
    if ref is None:
        raise SystemExit("the reference is not mounted: these fixtures can only be regenerated in the build container")
    arrays = {}
    with tempfile.TemporaryDirectory() as workdir:
        for case in CASES:
            layout, vals = record(ref, case, workdir)
            arrays[case[0] + ":layout"] = np.array(json.dumps(layout))
            arrays[case[0] + ":values"] = vals
            print(case[0], len(layout["events"]), "events", vals.size, "values",
                  sum(1 for e in layout["events"] if e[0] == "step" and e[2]), "episode ends")
    np.savez_compressed(TRACES, **arrays)

    shipped = {}
    for kind, rel in sorted(SHIPPED.items()):
        with open(os.path.join(_ref_harness.REFERENCE_DIR, rel)) as f:
            shipped[kind] = {"file": rel, "config": json.load(f)}
    with open(_ref_harness.REFERENCE_FILE) as f:
        src = f.read()
    with open(SHIPPED_CONFIGS, "w") as f:
        json.dump({"configs": shipped, "module_mentions": {k: k in src for k in INERT_KEYS}}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
