"""EpisodeMonitor / ProgressLog -- what stable-baselines' Monitor wrappers and the first job of the reference's training callback
do (examples/train_rl_controller.py monitor_training: log what the Monitors collected), on the device.

Monitor gives every finished episode its undiscounted return `r` and its length `l`; PPO2 logs their means over the last 100
episodes as ep_rewmean / eplenmean.  A training rollout here is a replayed hipGraph and its reward buffer holds VecNormalize'd
values, so FusedRollout(raw_rewards=True) has the step kernel write the raw reward of step t into row t of a buffer of its own
(no extra launch), and EpisodeMonitor.fold() folds that buffer and the done flags once per rollout (fwg_monitor_fold,
csrc/fwgym_monitor.h; include/fwgym.h "Training monitor").  Returns are summed as 64-bit integers in units of 2^-20, so the
result does not depend on wave order or on how the envs are sharded over ranks; the quantisation costs at most 2^-21 per step
(about 1e-3 over a 2 000-step episode in the worst case, far below what a logged mean needs).

ProgressLog is the log file: one row per update in <log_dir>/progress.csv, and every `log_interval` updates the reference's
printed block of the five info_kw measures per target state."""
import collections
import csv
import os

import numpy as np

from . import _native as nat

TAKE_KEYS = ("episodes", "nonfinite", "ep_rew_mean", "ep_len_mean", "ep_rew_min", "ep_rew_max", "ep_len_min", "ep_len_max")
MEASURES = ("success", "control_variation", "end_error", "total_error", "success_time_frac")


def combine(rows):
    """[ranks][8] doubles of fwg_monitor_take -> the 8 doubles of all ranks together: sums, minima, maxima."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, nat.N_MONITOR)
    return np.concatenate([rows[:, :4].sum(axis=0), [rows[:, 4].min(), rows[:, 5].max(), rows[:, 6].min(), rows[:, 7].max()]])


def summarize(total):
    """The 8 doubles -> the dictionary take() returns (None where no episode ended)."""
    n = int(total[0])
    some = n > 0
    return {"episodes": n, "nonfinite": int(total[1]),
            "ep_rew_mean": total[2] / n if some else None, "ep_len_mean": total[3] / n if some else None,
            "ep_rew_min": float(total[4]) if some else None, "ep_rew_max": float(total[5]) if some else None,
            "ep_len_min": int(total[6]) if some else None, "ep_len_max": int(total[7]) if some else None}


class EpisodeMonitor(object):
    """Return and length of the episodes of `vec` that end inside the rollouts handed to fold().  Owns the per-env carries (the
    open episode) and the kernel's scratch, on the env's memory backend; attaches itself to the env, whose reset() then abandons
    the open episodes of the envs it resets (Monitor(allow_early_resets=True))."""

    def __init__(self, vec, history=1024):
        if getattr(vec, "_monitor", None) is not None:
            raise RuntimeError("EpisodeMonitor: the env already has a monitor attached (detach() it first)")
        self.vec, self._lib, self.N = vec, vec._lib, int(vec.num_envs)
        m = vec._mem
        # (the backends have no 64-bit kinds: int64 and float64 words travel as pairs of 32-bit words)
        self.ep_q = m.zeros((self.N, 2), "i32")
        self.ep_len = m.zeros((self.N,), "i32")
        self.scratch = m.zeros((int(self._lib.fwg_monitor_scratch_bytes(self.N)) // 4,), "i32")   # all-zero: the identity
        self.out = m.zeros((2 * nat.N_MONITOR,), "i32")
        self._takes = collections.deque(maxlen=int(history))   # (episodes, sum_return, sum_length) of the latest takes
        vec._monitor = self

    def detach(self):
        if getattr(self.vec, "_monitor", None) is self:
            self.vec._monitor = None

    def fold(self, raw_rewards, dones):
        """One launch over a rollout's raw_rewards / dones ([T, N], step-major), stream-ordered behind whatever filled them."""
        T, N = int(raw_rewards.shape[0]), int(raw_rewards.shape[1])
        if N != self.N or tuple(dones.shape) != (T, N):
            raise ValueError("EpisodeMonitor.fold: raw_rewards {} / dones {} do not fit {} envs".format(
                tuple(raw_rewards.shape), tuple(dones.shape), self.N))
        m = self.vec._mem
        nat.check(self._lib, self._lib.fwg_monitor_fold(T, N, m.ptr(raw_rewards), m.ptr(dones), m.ptr(self.ep_q), m.ptr(self.ep_len),
                                                        m.ptr(self.scratch), m.stream()))

    def take_device(self):
        """fwg_monitor_take: the 8 doubles of the folds since the last take, left on the device (as 16 int32 words)."""
        m = self.vec._mem
        nat.check(self._lib, self._lib.fwg_monitor_take(self.N, m.ptr(self.scratch), m.ptr(self.out), m.stream()))
        return self.out

    def take(self, group=None):
        """The episodes that ended in the folds since the last take, of ALL ranks when torch.distributed is initialised (one
        all-gather of 64 B per rank: the device buffer under nccl, a host copy under gloo): {"episodes", "nonfinite",
        "ep_rew_mean", "ep_len_mean", "ep_rew_min", "ep_rew_max", "ep_len_min", "ep_len_max"}, None where no episode ended."""
        import torch
        import torch.distributed as dist
        m = self.vec._mem
        out = self.take_device()
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        if multi:
            use_dev = getattr(m, "device", None) is not None and dist.get_backend(group) == "nccl"
            t = out if use_dev else torch.as_tensor(np.ascontiguousarray(m.to_host(out)), dtype=torch.int32)
            gathered = torch.empty(dist.get_world_size(group) * t.numel(), dtype=torch.int32, device=t.device)
            dist.all_gather_into_tensor(gathered, t, group=group)
            rows = np.ascontiguousarray(gathered.cpu().numpy()).view(np.float64)
        else:
            rows = np.ascontiguousarray(m.to_host(out)).view(np.float64)
        total = combine(rows)
        self._takes.append((int(total[0]), float(total[2]), float(total[3])))
        return summarize(total)

    def window(self, k=100):
        """Means over the most recent takes that together hold at least `k` episodes (all kept takes when they hold fewer):
        stable-baselines' ep_info_buf of 100, at the granularity of a take.  {"episodes", "ep_rew_mean", "ep_len_mean"}."""
        n, ret, length = 0, 0.0, 0.0
        for episodes, sum_return, sum_length in reversed(self._takes):
            if n >= k:
                break
            n, ret, length = n + episodes, ret + sum_return, length + sum_length
        return {"episodes": n, "ep_rew_mean": ret / n if n else None, "ep_len_mean": length / n if n else None}

    def reset(self, indices=None):
        """Zeroes the carries (of the envs in `indices`): their open episodes are abandoned.  What has been folded stays."""
        if indices is None:
            self.ep_q[...] = 0
            self.ep_len[...] = 0
        else:
            idx = [int(i) for i in np.atleast_1d(indices)]
            self.ep_q[idx] = 0
            self.ep_len[idx] = 0

    def carries(self):
        """Host copies (ep_q int64 [N], ep_len int32 [N]) of the open episodes."""
        m = self.vec._mem
        return (np.ascontiguousarray(m.to_host(self.ep_q)).view(np.int64).reshape(self.N),
                np.array(m.to_host(self.ep_len), dtype=np.int32))


def flatten(info, prefix=""):
    """Scalars of a (nested) info dictionary as {"a/b": value}; anything that is not a number, a string or None is left out."""
    row = collections.OrderedDict()
    for key, value in info.items():
        name = prefix + str(key)
        if isinstance(value, dict):
            row.update(flatten(value, name + "/"))
        elif value is None or isinstance(value, (bool, int, float, str, np.integer, np.floating)):
            row[name] = value
    return row


class ProgressLog(object):
    """<log_dir>/progress.csv, one row per call (an update's info, flattened): the header comes from the first row's keys, later
    rows are written under the same keys and missing values stay empty.  Every `log_interval` calls the reference's block of
    info["ep_info"] is printed (train_rl_controller.py monitor_training): per measure, the mean per target state."""

    def __init__(self, log_dir, log_interval=50, out=print):
        self.log_dir, self.log_interval, self.out = log_dir, int(log_interval), out
        self.path = os.path.join(log_dir, "progress.csv")
        self.keys, self.rows = None, 0
        if not os.path.isdir(log_dir):
            os.makedirs(log_dir)

    @staticmethod
    def block(ep_info):
        """The reference's printed block, one string."""
        text = ""
        for measure in MEASURES:
            if measure in ep_info:
                text += "\n{}:\n\t".format(measure) + "\n\t".join(
                    "{:<10s}{:.2f}".format(state, mean) for state, mean in ep_info[measure].items() if mean is not None)
        return text

    def __call__(self, info):
        row = flatten(info)
        first = self.keys is None
        if first:
            self.keys = list(row)
        with open(self.path, "w" if first else "a", newline="") as f:
            w = csv.writer(f)
            if first:
                w.writerow(self.keys)
            w.writerow(["" if row.get(k) is None else row[k] for k in self.keys])
        self.rows += 1
        ep_info = info.get("ep_info")
        if self.out is not None and self.log_interval > 0 and self.rows % self.log_interval == 0 and ep_info and ep_info.get("episodes", 0) > 0:
            self.out(self.block(ep_info))
