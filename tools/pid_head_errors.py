#!/usr/bin/env python3
"""Where the bound of the PID-head tests comes from (tests/eval_device_common.py PID_TORCH_WORST): the worst absolute error
against float64 (oracle.pyfly_restated.PIDController) of the parent's BatchedPID -- torch fp32 on the CPU -- on the tests' own
open-loop inputs, per output and integrator and batch size; next to it the same figures of fwg_pid_act on the host emulation of the
kernels and, where a GPU is visible, on the device.

    python tools/pid_head_errors.py [--out profiles/pid_head_errors.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import eval_device_common as edc
    from emu.host_backend import HostBackend, build_emu
    from gym_fixed_wing import _native as nat
    keys = ("elevator", "aileron", "throttle", "int_roll", "int_pitch", "int_Va")
    paths = [("BatchedPID torch fp32 (CPU)", lambda n: edc.pid_torch_fp32(edc.pid_inputs(n)))]
    emu = (nat.load_library(build_emu()), HostBackend())
    paths.append(("fwg_pid_act, host emulation", lambda n: edc.run_pid(emu[0], emu[1], n)[:2]))
    if torch.cuda.is_available():
        from gym_fixed_wing.vec_env import _TorchBackend
        gpu = (nat.load_library(), _TorchBackend(0))
        paths.append(("fwg_pid_act, {}".format(torch.cuda.get_device_name(0)), lambda n: edc.run_pid(gpu[0], gpu[1], n)[:2]))
    lines = ["PID head: worst |error| against float64 over {} open-loop steps, gains {}".format(edc.PID_STEPS, edc.PID_GAINS),
             "torch {}".format(torch.__version__), "",
             "{:<34s} {:>5s} ".format("path", "N") + " ".join("{:>10s}".format(k) for k in keys) + "      worst"]
    worst = {}
    for name, fn in paths:
        for n in edc.PID_N:
            err = edc.pid_errors(*fn(n), edc.pid_inputs(n))
            worst[name] = max(worst.get(name, 0.0), max(err.values()))
            lines.append("{:<34s} {:>5d} ".format(name, n) + " ".join("{:>10.3e}".format(err[k]) for k in keys) + " {:>10.3e}".format(max(err.values())))
    lines += ["", "worst figure of the torch baseline: {:.4e}; asserted bound = min(2 x {:.4e}, 1e-3) = {:.4e}".format(
        worst[paths[0][0]], edc.PID_TORCH_WORST, edc.PID_BOUND)]
    for name in list(worst)[1:]:
        lines.append("{}: worst {:.4e} ({:.2f} of the bound)".format(name, worst[name], worst[name] / edc.PID_BOUND))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
