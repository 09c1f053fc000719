"""Batched baseline PID attitude/airspeed controller (device tensors).

The reference evaluates a PID baseline with `pyfly.pid_controller.PIDController`
(examples/evaluate_controller.py:6,82-84,120-124,143-150; fixed_wing.py:1281-1300), which is part of the absent PyFly
package; this is the same control law for N aircraft at once (gains as recalled in SURVEY.md App. B.2: roll PD on
(phi, p), pitch PID on (theta, q), PI airspeed -> throttle; outputs clipped to the actuator ranges)."""
import math


class BatchedPID(object):
    def __init__(self, n, dt=0.01, device=None):
        import torch
        self.torch = torch
        self.n, self.dt, self.device = n, dt, device
        self.k_p_V, self.k_i_V = 0.5, 0.1
        self.k_p_phi, self.k_i_phi, self.k_d_phi = 1.0, 0.0, 0.5
        self.k_p_theta, self.k_i_theta, self.k_d_theta = -4.0, -0.75, -0.1
        self.delta_a_min, self.delta_a_max = math.radians(-30), math.radians(30)
        self.delta_e_min, self.delta_e_max = math.radians(-30), math.radians(35)
        z = lambda: torch.zeros(n, dtype=torch.float32, device=device)
        self.phi_r, self.theta_r, self.va_r = z(), z(), z()
        self.int_va, self.int_roll, self.int_pitch = z(), z(), z()

    def reset(self, mask=None):
        for t in (self.int_va, self.int_roll, self.int_pitch):
            if mask is None:
                t.zero_()
            else:
                t[mask] = 0

    def set_reference(self, phi, theta, va):
        self.phi_r, self.theta_r, self.va_r = phi, theta, va

    def get_action(self, phi, theta, va, omega):
        torch = self.torch
        e_va, e_phi, e_theta = va - self.va_r, phi - self.phi_r, theta - self.theta_r
        p = omega[:, 0]
        q = omega[:, 1] * torch.cos(phi) - omega[:, 2] * torch.sin(phi)
        delta_a = -self.k_p_phi * e_phi - self.k_i_phi * self.int_roll - self.k_d_phi * p
        delta_e = -self.k_p_theta * e_theta - self.k_i_theta * self.int_pitch - self.k_d_theta * q
        delta_t = -self.k_p_V * e_va - self.k_i_V * self.int_va
        self.int_va = self.int_va + self.dt * e_va
        self.int_roll = self.int_roll + self.dt * e_phi
        self.int_pitch = self.int_pitch + self.dt * e_theta
        return torch.stack([delta_e.clamp(self.delta_e_min, self.delta_e_max),
                            delta_a.clamp(self.delta_a_min, self.delta_a_max), delta_t.clamp(0.0, 1.0)], dim=1)


PID_COLUMNS = ("roll", "pitch", "Va", "omega_p", "omega_q", "omega_r")


def default_gains(dt=0.01):
    """BatchedPID's gains and output limits as the fields of fwg_pid_gains."""
    return dict(k_p_phi=1.0, k_i_phi=0.0, k_d_phi=0.5, k_p_theta=-4.0, k_i_theta=-0.75, k_d_theta=-0.1, k_p_V=0.5, k_i_V=0.1,
                delta_e_min=math.radians(-30), delta_e_max=math.radians(35), delta_a_min=math.radians(-30),
                delta_a_max=math.radians(30), delta_t_min=0.0, delta_t_max=1.0, dt=dt)


class DevicePID(object):
    """The same control law as one HIP launch per step (fwg_pid_act, include/fwgym.h "Evaluation") on the buffers `vec`'s step
    kernel writes: the observation batch (vec._obs; for a row-log env the newest plane of the log, in place) and the target
    batch (vec._target, written by fwg_step(..., target_out): the reference refreshes the PID's reference from info["target"]
    after every step, evaluate_controller.py:146-149).  The integrators [3][N] (roll, pitch, Va) live in vec's memory backend,
    so the class serves the GPU and the host emulation of the kernels alike.  `gains`: fields of fwg_pid_gains that differ
    from BatchedPID's defaults."""

    def __init__(self, vec, gains=None):
        import ctypes
        from . import _native as nat
        self._nat, self._ctypes = nat, ctypes
        self.vec, self._lib, self._mem = vec, vec._lib, vec._mem
        obs_names = [v["name"] for v in vec.cfg["observation"]["states"]]
        try:
            cols = [obs_names.index(k) for k in PID_COLUMNS]
        except ValueError:
            raise ValueError("When using PID roll, pitch, Va, omega_p, omega_q, omega_r must be part of the "
                             "observation vector.")
        self._obs_cols = (ctypes.c_int32 * 6)(*cols)
        self._target_cols = (ctypes.c_int32 * 3)(*[vec.target_names.index(k) for k in ("roll", "pitch", "Va")])
        g = default_gains(vec.dt)
        unknown = set(gains or {}) - set(g)
        if unknown:
            raise TypeError("unknown PID gains: {}".format(sorted(unknown)))
        g.update(gains or {})
        self.gains = nat.PidGains(**{k: float(v) for k, v in g.items()})
        self.integrators = self._mem.zeros((3, vec.num_envs))

    def reset(self):
        self.integrators[...] = 0

    def act(self, out):
        """Actions [N][3] (elevator, aileron, throttle) for the observation `vec` currently shows into `out`; advances the
        integrators.  Stream-ordered, no host read."""
        vec, m = self.vec, self._mem
        obs = vec._obs
        if len(obs.shape) == 3:     # the row log's window [N][length][n_obs] (a strided view): its newest plane is dense [N][n_obs]
            obs = obs[:, 0]
        self._nat.check(self._lib, self._lib.fwg_pid_act(vec.num_envs, m.ptr(obs), int(obs.shape[1]), self._obs_cols, m.ptr(vec._target),
                                                         int(vec._target.shape[1]), self._target_cols, self.gains, m.ptr(self.integrators),
                                                         m.ptr(out), m.stream()))
        return out
