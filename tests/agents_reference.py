"""numpy float64 restatement of the per-drone race agents kernels (csrc/agents_kernel.h; include/adrp.h
adrp_race_agents_*), the yardstick of tests/test_agents_abi.py (pinned there by a case computed by hand and, for the
reward, against the oracle's RewardWrapper) and of the GPU tests.  Written from the reference's
utils/wrapper.py:121-186 (RewardWrapper.reset / _compute_reward) and the header's semantics, one agent slot
j = e * N + n at a time, in the order the header lists."""
import math

import numpy as np


def _cmod4(a):
    """C's a % 4 (the sign of the dividend), as the fused wrapper and the oracle compute it"""
    return int(math.fmod(int(a), 4))


class Agents:
    def __init__(self, E, N, D, num_gates):
        self.E, self.N, self.D, self.num_gates = int(E), int(N), int(D), int(num_gates)
        R = self.E * self.N
        self.wr_gate = np.zeros(R, np.int32)
        self.wr_target = np.zeros((R, 3), np.float64)
        self.wr_prev = np.zeros((R, 3), np.float64)
        self.alive = np.zeros(R, np.uint8)
        self.run_return = np.zeros(R, np.float64)
        self.run_length = np.zeros(R, np.int32)

    def reset(self, obs, mask=None):
        """RewardWrapper.reset per drone of the envs with mask[e] != 0 (None: all); nothing of another env is read"""
        rows = np.asarray(obs, np.float32).reshape(self.E * self.N, self.D)
        for j in range(self.E * self.N):
            if mask is not None and not mask[j // self.N]:
                continue
            row = rows[j]
            self.wr_gate[j] = int(row[48])
            self.wr_target[j] = row[12:15].astype(np.float64)
            self.wr_prev[j] = row[0:3].astype(np.float64)
            self.alive[j], self.run_return[j], self.run_length[j] = 1, 0.0, 0

    def step(self, obs, gate, flags, term, trunc, boot_value, gamma):
        """-> {"rewards" f32, "valid" u8, "next_start" f32, "ep_return" f64, "ep_length" i32, "raw" f64 (the
        reward before the bootstrap and the float32 rounding; NaN on a dead slot), "stored" f64 (with the bootstrap,
        before the rounding; 0 on a dead slot), "boot" bool}, each [E N]"""
        R = self.E * self.N
        rows = np.asarray(obs, np.float32).reshape(R, self.D)
        gate, flags = np.asarray(gate).reshape(R), np.asarray(flags).reshape(R)
        boot_value = np.asarray(boot_value, np.float32).reshape(R)
        out = {"rewards": np.zeros(R, np.float32), "valid": np.zeros(R, np.uint8), "next_start": np.zeros(R, np.float32),
               "ep_return": np.full(R, np.nan), "ep_length": np.zeros(R, np.int32), "raw": np.full(R, np.nan),
               "stored": np.zeros(R, np.float64), "boot": np.zeros(R, bool)}
        for j in range(R):
            e = j // self.N
            te, tr = bool(term[e]), bool(trunc[e])
            was_alive = bool(self.alive[j])
            done_now = (int(flags[j]) & 3) != 0
            fin = (int(flags[j]) & 2) != 0
            newly = was_alive and done_now
            out["valid"][j] = 1 if was_alive else 0
            out["next_start"][j] = 1.0 if (done_now or te or tr) else 0.0
            if not was_alive:
                continue                       # reward 0, NaN / 0 episode outputs, the state untouched
            row = rows[j].astype(np.float64)
            g = int(gate[j])
            r_passed = 0.0
            if g > _cmod4(self.wr_gate[j]):
                self.wr_gate[j] = g
                if 0 <= g < 4 and g < self.num_gates:
                    self.wr_target[j] = row[12 + 4 * g:15 + 4 * g]
                r_passed = 5.0
            r_col = -1.0 if (newly and not fin) else 0.0
            r_lap = 10.0 if (newly and fin) else 0.0
            tgt, prv = self.wr_target[j], self.wr_prev[j]
            pxy = math.sqrt((tgt[0] - prv[0]) * (tgt[0] - prv[0]) + (tgt[1] - prv[1]) * (tgt[1] - prv[1]))
            cxy = math.sqrt((tgt[0] - row[0]) * (tgt[0] - row[0]) + (tgt[1] - row[1]) * (tgt[1] - row[1]))
            pz, cz = abs(tgt[2] - prv[2]), abs(tgt[2] - row[2])
            r = (pxy - cxy) + (pz - cz) + r_passed + r_col + r_lap
            self.wr_prev[j] = row[0:3]
            boot = (not done_now) and tr and not te
            stored = r + float(gamma) * float(boot_value[j]) if boot else r
            out["raw"][j], out["stored"][j], out["boot"][j] = r, stored, boot
            out["rewards"][j] = np.float32(stored)
            self.run_return[j] += r
            self.run_length[j] += 1
            if newly or te or tr:
                out["ep_return"][j], out["ep_length"][j] = self.run_return[j], self.run_length[j]
            self.alive[j] = 0 if done_now else 1
        return out


def sequence(E, N, D=49, num_gates=4, T=6, seed=0):
    """A constructed stream of T steps for the array entry point: per step a dict of the step's inputs
    (obs [E N, D] float32, gate / flags int32 [E N], term / trunc uint8 [E], boot_value float32 [E N]) and of the
    reset that follows it (mask uint8 [E] = term | trunc, reset_obs [E N, D]); first the rows of the initial reset.
    It holds gate passes, gate == num_gates (the drone finishes), both flags on one drone, an elimination on the
    step its env is truncated, envs that end and are reset by the mask, and whole rows of NaN / Inf where a drone
    is dead (and as the stale boot_value of every env that is not truncated, and as the reset rows of every env
    that is not reset)."""
    rng = np.random.default_rng(seed)
    R = E * N

    def fresh_rows():
        rows = rng.uniform(-3, 3, (R, D)).astype(np.float32)
        rows[:, 2] = rng.uniform(0, 2, R).astype(np.float32)
        return rows

    def start_gate(j):
        return 1 if (j % 3 == 0 and num_gates > 1) else 0

    first = fresh_rows()
    gate = np.array([start_gate(j) for j in range(R)], np.int32)
    first[:, 48] = gate
    flags = np.zeros(R, np.int32)
    steps = []
    for t in range(T):
        dead_before = flags != 0
        trunc = np.array([(e + t) % 5 == 4 for e in range(E)], np.uint8)
        for j in range(R):
            if dead_before[j]:
                continue
            e, n = divmod(j, N)
            if (j * 7 + t * 3) % 11 == 0:
                gate[j] += 1
                if gate[j] >= num_gates:
                    gate[j] = num_gates
                    flags[j] |= 2
            if (j * 5 + t) % 13 == 0:
                flags[j] |= 1
            if j % 17 == 3 and t == 2:                       # both flags on one drone
                gate[j] = num_gates
                flags[j] = 3
            if trunc[e] and n == 0 and e % 2 == 1:           # eliminated on the step its env is truncated
                flags[j] |= 1
        term = np.array([bool((flags[e * N:(e + 1) * N] != 0).all()) for e in range(E)], np.uint8)
        obs = fresh_rows()
        obs[:, 48] = gate
        poison = np.where(np.arange(R) % 2 == 0, np.nan, np.inf).astype(np.float32)
        obs[dead_before] = poison[dead_before, None]
        boot_value = rng.uniform(-4, 4, R).astype(np.float32)
        boot_value[np.repeat(trunc == 0, N)] = np.nan
        step = dict(obs=obs, gate=gate.copy(), flags=flags.copy(), term=term, trunc=trunc, boot_value=boot_value,
                    dead_before=dead_before)
        mask = (term | trunc).astype(np.uint8)
        reset_obs = fresh_rows()
        slots = np.repeat(mask != 0, N)
        for j in np.nonzero(slots)[0]:
            gate[j], flags[j] = start_gate(j), 0
        reset_obs[:, 48] = gate
        reset_obs[~slots] = np.nan
        step.update(mask=mask, reset_obs=reset_obs)
        steps.append(step)
    return first, steps
