#!/usr/bin/env python3
"""Times one whole off-policy update (critic step, actor step, Polyak pass) of DDPG(update="hip") and of DDPG(update="torch") on the
same batch in the same process, and each call of the HIP path on its own, at (D, G, A) = (11, 3, 3), B = 4 096 and 65 536, one and two
critics.  One fresh process per run, medians of `--runs` runs; inside a run a warm-up, then alternating blocks per figure, device time
by events.  The feature has no earlier version: the torch path in the same process is the baseline.

  update_us        one DDPG.update(batch) as a user calls it, statistics read back (the call waits for the device)
  step_us          HIP only: fwg_ddpg_step issued back to back, no read-back -- what the launches themselves cost
  critic_grad_us   k_ddpg_critic_grad + k_ddpg_reduce;  actor_grad_us  k_ddpg_actor_grad + k_ddpg_reduce
  apply_us         k_ddpg_apply on the critics' segment; apply_polyak_us  k_ddpg_apply on the actor's segment + k_ddpg_polyak
beside each gradient call its algorithmic bytes and FLOPs per row (one pass over the batch, every product counted once: the hi + lo
split triples the matrix-core work) and the time either bound would allow on 8 TB/s and 2.5 PFLOP/s (bf16, dense).

    timeout -k 10 900 python tools/time_offpolicy_update.py --out profiles/offpolicy_update_timing.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]

D, G, A = 11, 3, 3
CASES = [(4096, 1), (4096, 2), (65536, 1), (65536, 2)]
HBM_BYTES_PER_S, BF16_FLOPS = 8.0e12, 2.5e15


def net_flops(K, nout, backward):
    """Multiply-adds x 2 of one 64-64 network on one row: forward, and (backward) the weight gradients and the hidden-side gradients."""
    fwd = 2 * (64 * K + 64 * 64 + 64 * nout)
    return fwd + (2 * (2 * 64 * 64 + 64 * K + 2 * 64 * nout) if backward else 0)


def per_row(nc):
    Ka, Kc = D + G, D + G + A
    critic = {"bytes": 4 * (2 * D + 4 + A + 1) + 1,   # o, o', the 4-word goal row, a, r, done
              "flops": net_flops(Ka, A, False) + nc * net_flops(Kc, 1, False) + nc * net_flops(Kc, 1, True)}
    # (the actor launch: pi, Q_0, back through the critic for dQ / da -- two 64 x 64 products' worth less than a full backward -- and the actor)
    actor = {"bytes": 4 * (D + 4), "flops": net_flops(Ka, A, True) + net_flops(Kc, 1, False) + 2 * (64 * 64 + 64 + 64 * A)}
    return critic, actor


def timed(call, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def child():
    import torch
    from gym_fixed_wing import _native as nat
    from gym_fixed_wing.offpolicy import DDPG
    dev = torch.device("cuda", 0)
    out = {}
    for B, nc in CASES:
        g = torch.Generator().manual_seed(B + nc)
        rows = torch.zeros(B, 4)
        rows[:, :G] = torch.randn(B, G, generator=g)
        batch = {"observation": torch.randn(B, D, generator=g) * 1.5, "next_observation": torch.randn(B, D, generator=g) * 1.5,
                 "action": torch.rand(B, A, generator=g) * 2 - 1, "desired_rows": rows, "reward": torch.randn(B, generator=g),
                 "done": (torch.rand(B, generator=g) < 0.25).to(torch.uint8)}
        batch = {k: v.to(dev).contiguous() for k, v in batch.items()}
        agents = {p: DDPG(D, G, A, n_critics=nc, update=p, device=dev, seed=0) for p in ("hip", "torch")}
        L = agents["hip"].updater
        bs, u = L.batch_struct(batch), [1]

        def step():
            p = lambda t: nat.C.c_void_p(int(t.data_ptr()))
            nat.check(L._lib, L._lib.fwg_ddpg_step(L._h, nat.C.byref(bs), B, u[0], 1, nat.C.byref(L.hparams), p(L.flat), p(L.target), p(L.exp_avg),
                                                   p(L.exp_avg_sq), p(L.steps), p(L.stats), L._stream()))
            u[0] += 1
        calls = {"hip_update_us": (lambda: agents["hip"].update(batch), 20), "torch_update_us": (lambda: agents["torch"].update(batch), 20),
                 "hip_step_us": (step, 50),
                 "critic_grad_us": (lambda: L.critic_grad(bs, B, L.grad), 50), "actor_grad_us": (lambda: L.actor_grad(bs, B, L.grad), 50),
                 "apply_us": (lambda: L.apply(nat.DDPG_CRITICS, L.grad, B), 50),
                 "apply_polyak_us": (lambda: L.apply(nat.DDPG_ACTOR, L.grad, B, polyak=True), 50)}
        for call, _ in calls.values():   # warm-up: code objects, allocator, Adam's state
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(5):   # alternating blocks
            for k, (call, reps) in calls.items():
                us[k].append(timed(call, reps))
        out["B{}_critics{}".format(B, nc)] = {k: statistics.median(v) for k, v in us.items()}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()
    rows = []
    for _ in range(args.runs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], check=True, capture_output=True, text=True)
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"shape": {"obs_dim": D, "goal_dim": G, "act_dim": A},
           "method": "one fresh process per run, medians of {} runs; inside a run a warm-up of 3 calls, then 5 alternating blocks of 20 (updates) "
                     "or 50 (single calls) calls per figure, device events".format(args.runs), "cases": {}}
    for case in rows[0]:
        B, nc = int(case.split("_")[0][1:]), int(case[-1])
        c = {k: {"median": statistics.median(r[case][k] for r in rows), "min": min(r[case][k] for r in rows), "max": max(r[case][k] for r in rows)}
             for k in rows[0][case]}
        c["speedup_update"] = c["torch_update_us"]["median"] / c["hip_update_us"]["median"]
        for name, pr in zip(("critic_grad", "actor_grad"), per_row(nc)):
            c[name + "_per_row"] = dict(pr, memory_bound_us=B * pr["bytes"] / HBM_BYTES_PER_S * 1e6,
                                        matrix_bound_us_split3=3 * B * pr["flops"] / BF16_FLOPS * 1e6)
        out["cases"][case] = c
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
