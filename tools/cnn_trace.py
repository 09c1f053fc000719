#!/usr/bin/env python3
"""Settles the two things the shipped CNN checkpoint does not record (tests/golden/cnn_controller.npz; the reference's
examples/models/cnn_controller, trained by train_rl_controller.py --policy CNN, :179-197):

  A  the activation after the 5 x 1 conv: identity, tanh or relu
  F  the flatten order of its 12 x 3 output: feature-major j*3 + c (TF's NHWC reshape, SB2's conv_to_fc) or filter-major c*12 + j

Each of the six (A, F) candidates flies the 100 shipped no-wind scenarios on the float64 oracle through the reference's evaluation
protocol (examples/evaluate_controller.py:44-169, incl. the UN-normalised first observation of every episode) and is scored
against the published per-step rewards (tests/golden/eval_res_RL_CNN_none_rewards.npz) and the published CNN table row.

    python tools/cnn_trace.py [--candidates identity:nhwc,tanh:nhwc,...] [--scenarios 100] [--jobs 8]

CPU only; ~1 min per candidate on 8 cores.  Writes the table to profiles/cnn_architecture.txt."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mlp_trace as mt  # noqa: E402
import structure_scan as ss  # noqa: E402

_Z = np.load(os.path.join(ROOT, "tests", "golden", "cnn_controller.npz"))
_W = {k[2:]: _Z[k].astype(np.float64) for k in _Z.files if k.startswith("w_")}
_MEAN = _Z["obs_rms_mean"].astype(np.float64)
_STD = np.sqrt(_Z["obs_rms_var"].astype(np.float64) + 1e-8)
ACTS = {"identity": lambda z: z, "tanh": np.tanh, "relu": lambda z: np.maximum(z, 0.0)}
ORDERS = ("nhwc", "chw")


def policy_mean(x, act, order):
    """x: (5, 12) -> mean action of candidate (act, order), float64."""
    w = _W["c1_w"][:, 0, 0, :]                        # [rows][filters]
    y = ACTS[act](x.T @ w + _W["c1_b"].reshape(-1))    # [12 features][3 filters]
    feat = y.reshape(-1) if order == "nhwc" else y.T.reshape(-1)
    h = np.tanh(feat @ _W["pi_fc0_w"] + _W["pi_fc0_b"])
    h = np.tanh(h @ _W["pi_fc1_w"] + _W["pi_fc1_b"])
    return h @ _W["pi_w"] + _W["pi_b"]


def fly(args):
    """(candidate (act, order), scenario, config, tmpdir[, max_steps]) -> (rewards, final info)."""
    cand, sc, cfg, tmpdir = args[:4]
    max_steps = args[4] if len(args) > 4 else None
    act, order = cand
    import oracle.gym_restated as gr
    from gym_fixed_wing import evaluate as ev
    from oracle.gym_restated import FixedWingOracle
    v = ss.parse_variant("base")
    pp, sp = ss.build_files(v, tmpdir)
    ss.VariantPyFly.variant = v
    gr.PyFly = ss.VariantPyFly
    env = FixedWingOracle(cfg, config_kw=ev.evaluation_overrides(False), sim_config_kw={"turbulence": False, "turbulence_intensity": "none"},
                          sim_config_path=sp, sim_parameter_path=pp)
    obs = env.reset(state=sc["state"], target=sc["target"])
    rews, done, first, info = [], False, True, None
    while not done:
        x = np.asarray(obs, dtype=np.float64).reshape(5, 12)
        xn = x if first else np.clip((x - _MEAN) / _STD, -10.0, 10.0)   # evaluate_controller.py:118: raw first observation
        first = False
        obs, r, done, info = env.step(policy_mean(xn, act, order))
        rews.append(float(r))
        if max_steps is not None and len(rews) >= max_steps:
            break
    return rews, {k: info.get(k) for k in ("termination", "settling_time", "rise_time", "control_variation", "success", "overshoot")}


def published(n=None):
    """tests/golden/eval_res_RL_CNN_none_rewards.npz in the layout mlp_trace.score reads: per-episode reward lists (the first 100
    steps), episode lengths, the table; the first `n` episodes."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "eval_res_RL_CNN_none_rewards.npz"))
    lens = z["episode_lengths"][:n]
    return {"rewards": [r[:min(int(m), r.size)].astype(np.float64).tolist() for r, m in zip(z["rewards"][:n], lens)],
            "episode_lengths": lens.tolist(),
            "table": {"settling_time_s": {k: float(z["settling_" + k]) for k in ("roll", "pitch", "Va")},
                      "control_variation": float(z["control_variation"])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default=",".join("{}:{}".format(a, o) for o in ORDERS for a in ACTS))
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--jobs", type=int, default=max(1, min(8, os.cpu_count() or 1)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_architecture.txt"))
    args = ap.parse_args()
    import configs
    import multiprocessing as mp
    cfg = configs.reference_like("cnn")
    with open(os.path.join(ROOT, "tests", "golden", "test_set_wind_none.json")) as f:
        scen = json.load(f)[:args.scenarios]
    pub = published(len(scen))
    tmpdir = tempfile.mkdtemp()
    lines = ["# tools/cnn_trace.py: the six (activation A, flatten order F) readings of the shipped CNN checkpoint flown on the",
             "# float64 oracle, {} no-wind scenarios, reference evaluation protocol (raw first observation).".format(len(scen)),
             "# |dr|: per-step reward error against eval_res_RL_CNN_none (first 100 steps of every episode).",
             "# published: success 100/100/100/100, settling {:.3f}/{:.3f}/{:.3f} s, control variation {:.3f}".format(
                 pub["table"]["settling_time_s"]["roll"], pub["table"]["settling_time_s"]["pitch"], pub["table"]["settling_time_s"]["Va"],
                 pub["table"]["control_variation"]),
             "{:>16s} {:>6s} {:>6s} {:>6s} {:>6s}  {:>20s} {:>6s} {:>8s} {:>8s} {:>8s} {:>6s}".format(
                 "candidate", "succ", "roll", "pitch", "Va", "settling r/p/Va", "cv", "|dr|mean", "|dr|p90", "r1 err", "len")]
    with mp.get_context("fork").Pool(args.jobs) as pool:
        for name in args.candidates.split(","):
            act, order = name.split(":")
            res = pool.map(fly, [((act, order), sc, cfg, tmpdir) for sc in scen], chunksize=1)
            s = mt.score(res, pub)
            s["success_%"] = {k: 100.0 * float(np.mean([bool(i["success"][k]) for _, i in res])) for k in ("roll", "pitch", "Va", "all")}
            st = s["settling_s"]
            lines.append("{:>16s} {:6.0f} {:6.0f} {:6.0f} {:6.0f}  {:6.3f}/{:6.3f}/{:6.3f} {:6.3f} {:8.4f} {:8.4f} {:8.4f} {:6.3f}".format(
                name, s["success_%"]["all"], s["success_%"]["roll"], s["success_%"]["pitch"], s["success_%"]["Va"], st["roll"], st["pitch"],
                st["Va"], s["control_variation"], s["mean_abs_dreward_first100"], s["p90_abs_dreward_first100"],
                s["second_step_reward_abs_err"], s["episode_length_ratio_median"]))
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
