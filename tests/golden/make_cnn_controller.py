#!/usr/bin/env python3
"""Generates tests/golden/cnn_controller.npz and tests/golden/eval_res_RL_CNN_none_rewards.npz from a checkout of the reference.

Inputs: the reference's shipped CNN policy (gym_fixed_wing/examples/models/cnn_controller/{model.pkl, obs_rms.pkl, ret_rms.pkl},
trained by examples/train_rl_controller.py --policy CNN) and its published evaluation on the no-wind test set
(examples/evaluations/eval_res_RL_CNN_none.npy).  model.pkl is stable-baselines' cloudpickle of (data, params): it is read with
a RESTRICTED unpickler -- only numpy's array reconstruction, `_codecs.encode` and `collections.OrderedDict` resolve; every
cloudpickle / stable_baselines / gym global becomes an inert stub, so nothing of the training code is imported or executed.

Outputs (plain arrays, np.load without pickles):
  cnn_controller.npz                  w_<name>: weights in TF layout ([in][out] kernels, conv kernel [rows][cols][in][out]);
                                      obs_rms_{mean,var,count} (mean / var 5 x 12), ret_rms_{mean,var,count}, ppo2_<hyper-parameter>,
                                      n_filters (policy_kwargs), observation_shape, published_episode_lengths
  eval_res_RL_CNN_none_rewards.npz    rewards [episode][step]: the first 100 rewards per episode un-normalised with this model's
                                      ret_rms (the evaluation runs VecNormalize(training=False), evaluate_controller.py:93-100),
                                      NaN past an episode's end; episode_lengths, reward_scale; the table: success_<state> (%),
                                      settling_<state> / rise_<state> (s, over successful episodes), control_variation

    python tests/golden/make_cnn_controller.py <reference checkout>/gym_fixed_wing/examples
"""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KEEP = 100


class _Stub(object):
    """Inert stand-in for every global outside the allow-list: takes any arguments and any state, does nothing."""

    def __new__(cls, *a, **k):
        return object.__new__(cls)

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Stub()

    def __setstate__(self, state):
        self.state = state

    def __setitem__(self, k, v):
        pass


class _Restricted(pickle.Unpickler):
    ALLOWED = {("numpy.core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"), ("numpy", "ndarray"),
               ("numpy", "dtype"), ("_codecs", "encode"), ("collections", "OrderedDict")}

    def find_class(self, module, name):
        if (module, name) in self.ALLOWED:
            if module == "numpy.core.multiarray":
                import numpy.core.multiarray as m
                return getattr(m, name)
            return super().find_class(module, name)
        if module.split(".")[0] in ("cloudpickle", "stable_baselines", "gym", "builtins", "copyreg", "types"):
            return type(name, (_Stub,), {})
        raise pickle.UnpicklingError("global {}.{} is not allowed".format(module, name))


def _load(path):
    with open(path, "rb") as f:
        return _Restricted(f).load()


def _rms(path):
    o = _load(path)
    st = o.state if hasattr(o, "state") else o.__dict__
    return {"mean": np.asarray(st["mean"], np.float64), "var": np.asarray(st["var"], np.float64), "count": float(st["count"])}


def main(ref):
    model = os.path.join(ref, "models", "cnn_controller")
    data, params = _load(os.path.join(model, "model.pkl"))
    w = {k.replace("model/", "").replace(":0", "").replace("/", "_"): np.asarray(v, np.float32) for k, v in params.items()}
    w.pop("q_w", None), w.pop("q_b", None)   # SB2's unused q head
    obs_rms, ret_rms = _rms(os.path.join(model, "obs_rms.pkl")), _rms(os.path.join(model, "ret_rms.pkl"))
    space = data["observation_space"]
    shape = list(space.state["shape"]) if hasattr(space, "state") and isinstance(space.state, dict) else [5, 12]
    hp = {k: data[k] for k in ("gamma", "n_steps", "vf_coef", "ent_coef", "max_grad_norm", "lam", "nminibatches", "noptepochs",
                               "n_envs", "num_timesteps") if k in data}
    hp["cliprange"] = data["cliprange"] if isinstance(data.get("cliprange"), float) else 0.2   # (a constfn closure in the file)
    pub = np.load(os.path.join(ref, "evaluations", "eval_res_RL_CNN_none.npy"), allow_pickle=True).item()
    out = {"w_" + k: v for k, v in w.items()}
    out.update({"obs_rms_mean": obs_rms["mean"], "obs_rms_var": obs_rms["var"], "obs_rms_count": obs_rms["count"],
                "ret_rms_mean": ret_rms["mean"], "ret_rms_var": ret_rms["var"], "ret_rms_count": ret_rms["count"],
                "n_filters": int((data.get("policy_kwargs") or {})["n_filters"]), "observation_shape": np.array(shape),
                "published_episode_lengths": np.array([len(r) for r in pub["rewards"]])})
    out.update({"ppo2_" + k: v for k, v in hp.items()})
    np.savez_compressed(os.path.join(HERE, "cnn_controller.npz"), **out)
    scale = float(np.sqrt(float(ret_rms["var"]) + 1e-8))
    assert max(abs(x) for r in pub["rewards"] for x in r) < 9.9, "a stored reward sits at the VecNormalize clip"
    ok = np.array([bool(v) for v in pub["success"]["all"]])
    mean_ok = lambda v, s: float(np.nanmean(np.where(ok, np.array([np.nan if x is None else x for x in v], dtype=float), np.nan))) * s
    rewards = np.full((len(pub["rewards"]), KEEP), np.nan, np.float32)
    for i, r in enumerate(pub["rewards"]):
        rewards[i, :min(len(r), KEEP)] = np.asarray(r[:KEEP], np.float64) * scale
    rew = {"rewards": rewards, "episode_lengths": np.array([len(r) for r in pub["rewards"]]), "reward_scale": scale,
           "control_variation": mean_ok(pub["control_variation"]["all"], 1.0)}
    for k, v in pub["success"].items():
        rew["success_" + k] = 100.0 * float(np.mean([bool(x) for x in v]))
    for k, v in pub["settling_time"].items():
        rew["settling_" + k] = mean_ok(v, 0.01)
    for k, v in pub["rise_time"].items():
        rew["rise_" + k] = mean_ok(v, 0.01)
    np.savez_compressed(os.path.join(HERE, "eval_res_RL_CNN_none_rewards.npz"), **rew)
    print("weights", {k: v.shape for k, v in w.items()}, "obs", shape, "ppo2", hp)
    print("scale", scale, {k: v for k, v in rew.items() if np.ndim(v) == 0})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
