#!/usr/bin/env python3
"""The measured errors behind the tolerances of tests/goal_common.py (REWARD_TOL, GOLDEN_TOL, ANCHOR_TOL): the bodies of the goal
tests run once with the assertions on the bounds lifted to their caps, and the worst figure of each is printed.

    python tools/goal_errors.py emu          # host emulation of the kernels
    python tools/goal_errors.py gpu          # the device

profiles/goal_errors.txt keeps the output of both."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "tests")]


def main():
    backend = sys.argv[1] if len(sys.argv) > 1 else "emu"
    import goal_common as gc
    if backend == "emu":
        from emu.host_backend import HostBackend, build_emu
        kw = {"_backend": HostBackend(), "_lib_path": build_emu()}
    else:
        kw = {"device": 0}
    gc.REWARD_TOL = 1e-5   # the cap: this run measures
    print("goal errors, backend {}".format(backend))
    worst = 0.0
    for kind in gc.KINDS:
        w = max(gc.reward_contract(kw, kind, m) for m in gc.CONTRACT_M)
        worst = max(worst, w)
        print("  fwg_goal_reward vs float64 restatement, {:22s} worst |got - want| / max(1, |want|) over m {}: {:.3e}".format(kind, gc.CONTRACT_M, w))
    for n in gc.RELABEL_N:
        vec = gc.make_env(kw, gc.goal_config("reward_mix_potential"), n)
        ref = gc.RefReward(vec)
        for t in gc.RELABEL_T:
            gc.relabel_cell(vec, ref, t)
        vec.close()
    print("  fwg_goal_relabel relabelled rewards vs restatement, reward_mix_potential, T x N grid:            {:.3e}".format(gc.WORST["relabel"]))
    print("  reward function, worst of both:                                                                  {:.3e}".format(max(worst, gc.WORST["relabel"])))
    for form in ("absolute", "potential"):
        print("  fwg_goal_reward mode 0 vs recorded reference rewards (g4_goal_{}.json), worst |got - want|: {:.3e}".format(form, gc.reward_golden(kw, form)))
    for form in ("absolute", "potential"):
        print("  fwg_goal_reward mode 1 on own goals vs the step's raw reward, {:9s} worst |got - want|:       {:.3e}".format(form, gc.anchor_to_the_step(kw, form)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
