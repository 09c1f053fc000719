#!/usr/bin/env python3
"""Evaluation protocol of the reference (examples/evaluate_controller.py:44-169 there) on the MI355X env: flies a test
set of (initial state, target) scenarios, all scenarios in one batch, with the PID baseline or a stable-baselines MLP
policy or the CnnMlpPolicy of the shipped CNN controller (both through the HIP rollout head), and prints the table of
examples/README.md:33-47.  For the CNN controller the first action of every episode is computed from the un-normalised reset
observation, as the reference's script does (evaluate_controller.py:118 there; the protocol its published CNN row carries).

    python examples/evaluate_controller.py --controller pid
    python examples/evaluate_controller.py --controller mlp --model tests/golden/mlp_controller.json
    python examples/evaluate_controller.py --controller cnn     (model: tests/golden/cnn_controller.npz)
    python examples/evaluate_controller.py --controller cnn --device-loop     (the loop on the device; any controller)

Test-set format: JSON list of {"state": {...}, "target": {...}} (converted from the reference's .npy test sets; the one
under tests/golden/ is its examples/test_sets/test_set_wind_none_step20-20-3.npy)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]

from gym_fixed_wing import evaluate as ev, presets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--controller", default="pid", choices=["pid", "mlp", "cnn"])
    ap.add_argument("--test-set", default=os.path.join(ROOT, "tests", "golden", "test_set_wind_none.json"))
    ap.add_argument("--model", default=None,
                    help="converted checkpoint (actor.load_controller): stable-baselines MlpPolicy / CnnMlpPolicy weights and obs_rms; "
                         "default tests/golden/mlp_controller.json / cnn_controller.npz")
    ap.add_argument("--turbulence", default="none", choices=["none", "light", "moderate", "severe"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--device-loop", action="store_true",
                    help="run the protocol's loop on the device (evaluate.evaluate_on_set_device: no host read per step); same table")
    args = ap.parse_args()
    with open(args.test_set) as f:
        scenarios = json.load(f)
    if args.controller == "pid" and args.device_loop:
        t = ev.evaluate_on_set_device(scenarios, presets.preset("examples"), turbulence_intensity=args.turbulence, device=args.device).table()
    elif args.controller == "pid":
        res = ev.evaluate_on_set(scenarios, presets.preset("examples"), turbulence_intensity=args.turbulence, device=args.device)
    else:
        import numpy as np
        from gym_fixed_wing.actor import DeviceActor, load_controller, module_from_weights, weights_from_stable_baselines
        model = args.model or os.path.join(ROOT, "tests", "golden", "mlp_controller.json" if args.controller == "mlp" else "cnn_controller.npz")
        m = load_controller(model)
        w = weights_from_stable_baselines(m["weights"])
        obs_dim = int(np.asarray(m["obs_rms"]["mean"]).size)
        actor = DeviceActor(len(scenarios), obs_dim, training=False, device=args.device)
        actor.load_policy(w)
        actor.set_stats(np.asarray(m["obs_rms"]["mean"]).reshape(-1), np.asarray(m["obs_rms"]["var"]).reshape(-1), 1e6)
        first = None
        if "c1_w" in w:   # the first action of an episode: the same network on the raw observation (torch fp32)
            net = module_from_weights(w, np.asarray(m["obs_rms"]["mean"]).shape).to("cuda:{}".format(args.device))
            first = lambda obs: net.pi(obs.reshape(obs.shape[0], -1))
        if args.device_loop:
            t = ev.evaluate_on_set_device(scenarios, presets.preset(args.controller), controller=actor, turbulence_intensity=args.turbulence,
                                          device=args.device, first_step_policy=first).table()
        else:
            res = ev.evaluate_on_set(scenarios, presets.preset(args.controller), turbulence_intensity=args.turbulence, device=args.device,
                                     policy=lambda obs: actor.act(obs.reshape(obs.shape[0], -1).contiguous(), deterministic=True)[1],
                                     first_step_policy=first)
    if not args.device_loop:
        t = ev.summarize(res)
    print("controller {}, {} scenarios, turbulence {}".format(args.controller, len(scenarios), args.turbulence))
    print("success %      roll {roll:6.1f}  pitch {pitch:6.1f}  Va {Va:6.1f}  all {all:6.1f}".format(**t["success_%"]))
    for k, unit in (("rise_time", "s"), ("settling_time", "s"), ("overshoot", "%")):
        print("{:<14s} roll {:6.3f}  pitch {:6.3f}  Va {:6.3f}  [{}]".format(k, t[k]["roll"], t[k]["pitch"], t[k]["Va"], unit))
    print("control variation {:.3f}".format(t["control_variation"]["all"]))


if __name__ == "__main__":
    main()
