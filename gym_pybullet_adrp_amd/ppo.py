"""On-device PPO update (the learner half of examples/learn.py:72-94, ``model.learn``).

``PPOLearner`` is stable_baselines3 2.3.2 ``PPO.train()`` for the ``MlpPolicy`` a ``DevicePolicy``
serves (actor, separate critic, state-independent ``log_std``), restated from SB3's published code:
per minibatch the clipped-surrogate loss, its gradient with respect to the 13 parameter tensors,
``clip_grad_norm_`` and ``torch.optim.Adam(eps=1e-5)``, in four HIP launches on the tensors a
``RolloutCollector`` already holds (csrc/ppo_kernel.h).  Each update rewrites the attached policy's
device weights in place, so the next ``collect()`` samples from the updated policy; nothing
synchronises with the host.

``target_kl`` is SB3's early stop (``approx_kl_div > 1.5 * target_kl``: skip that minibatch's optimizer
step, leave the minibatch and the epoch loop) as a latch in the learner's device memory: the reduce launch
that computes the minibatch's KL sets it, the launches of every later minibatch read it and return, so
``train`` still issues every launch and reads nothing back (``stop_info()`` is the one deliberate read).
It is switched on with ``learner.set_target_kl(x)``, the C-ABI's setter; the ``target_kl=`` keyword of the
constructor and of ``train`` stays refused, as before the latch was built.
``learning_rate``, ``clip_range`` and ``clip_range_vf`` take a float or a callable of
``progress_remaining`` (1 at the start of training, 0 at its end), evaluated once at the head of each
``train`` as SB3 does; ``linear_schedule`` is SB3's ``get_linear_fn``.
"""
import ctypes

import torch

from . import _lib
from .policy import ACTOR_KEYS, CRITIC_KEYS
from .utils import abi

KEYS = ACTOR_KEYS + CRITIC_KEYS
STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")
_NO_KEYWORD = ("target_kl is not taken here: the early stop is a latch on the device, switch it on with "
               "PPOLearner.set_target_kl()")


def linear_schedule(start, end=0.0, end_fraction=1.0):
    """SB3's ``get_linear_fn``: a callable of ``progress_remaining`` that goes from ``start`` (at 1) to ``end``,
    reached after the fraction ``end_fraction`` of training, and stays there"""
    start, end, end_fraction = float(start), float(end), float(end_fraction)

    def func(progress_remaining):
        if (1 - progress_remaining) > end_fraction:
            return end
        return start + (1 - progress_remaining) * (end - start) / end_fraction

    return func


def _rate(x, progress_remaining):
    return float(x(progress_remaining)) if callable(x) else float(x)


class PPOLearner:
    """SB3 ``PPO.train()`` on the device for ``policy`` (a ``DevicePolicy`` with a critic).  The
    learner must be closed (or dropped) before its policy, and the policy's ``set_critic`` must not
    be called while a learner is attached."""

    target_kl = None        # no early stop, constant rates: the state before __init__ sets them
    _scheduled = False
    _nmb = 0

    def __init__(self, policy, learning_rate=3e-4, n_epochs=10, batch_size=64, clip_range=0.2, clip_range_vf=None,
                 normalize_advantage=True, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, seed=0, target_kl=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.AdrpError("no HIP device visible: libadrp has no CPU fallback")
        if target_kl is not None:
            raise ValueError(_NO_KEYWORD)
        if int(n_epochs) < 1 or int(batch_size) < 1:
            raise ValueError("n_epochs and batch_size must be at least 1")
        self.policy = policy
        self.n_epochs, self.batch_size = int(n_epochs), int(batch_size)
        cfg = abi.AdrpPpoCfg()
        self.lib.adrp_ppo_default_cfg(ctypes.byref(cfg))
        # the rates at the start of training; a callable is evaluated again at the head of every train()
        self.learning_rate, self.clip_range, self.clip_range_vf = learning_rate, clip_range, clip_range_vf
        cfg.learning_rate, cfg.clip_range = _rate(learning_rate, 1.0), _rate(clip_range, 1.0)
        cfg.clip_range_vf = -1.0 if clip_range_vf is None else _rate(clip_range_vf, 1.0)
        cfg.normalize_advantage = int(bool(normalize_advantage))
        cfg.ent_coef, cfg.vf_coef, cfg.max_grad_norm = float(ent_coef), float(vf_coef), float(max_grad_norm)
        if clip_range_vf is not None and cfg.clip_range_vf < 0:
            raise ValueError("clip_range_vf must not be negative")
        h = ctypes.c_void_p()
        rc = self.lib.adrp_ppo_create(getattr(policy, "h", None), ctypes.byref(cfg), ctypes.byref(h))
        if rc != 0:
            msg = self.lib.adrp_last_error(None).decode()
            raise (ValueError if rc == abi.ERR_INVALID else _lib.AdrpError)(msg)
        self.h, self.cfg = h, cfg
        self.device = policy.device
        self.total = self.lib.adrp_ppo_param_count(h)
        A, D, H1, H2 = policy.act_dim, policy.in_dim, policy.h1, policy.h2
        net = lambda out: [(H1, D), (H1,), (H2, H1), (H2,), (out, H2), (out,)]
        self.shapes = dict(zip(KEYS, net(A) + net(1) + [(A,)]))
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        self._stats = torch.zeros(5, dtype=torch.float32, device=self.device)
        self._scheduled = any(callable(x) for x in (learning_rate, clip_range, clip_range_vf))
        self.stop_state = torch.zeros(2, dtype=torch.int32, device=self.device)   # (tripped, optimizer steps applied)
        self._nmb = 0
        self.set_target_kl(None)

    # ---- flat vector <-> {SB3 key: tensor} ----
    def _split(self, flat):
        out, o = {}, 0
        for k in KEYS:
            n = 1
            for s in self.shapes[k]:
                n *= s
            out[k] = flat[o:o + n].view(self.shapes[k])
            o += n
        assert o == self.total
        return out

    def _join(self, sd):
        return torch.cat([torch.as_tensor(sd[k]).to(device=self.device, dtype=torch.float32).reshape(-1) for k in KEYS])

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.adrp_last_error(None).decode()
            raise (ValueError if rc == abi.ERR_INVALID else _lib.AdrpError)(f"{what}: {msg}")

    def _flat(self):
        return torch.empty(self.total, dtype=torch.float32, device=self.device)

    def _stream(self):
        return _lib._raw_stream(self.device.index)

    def state_dict(self):
        """the 13 tensors under SB3's key names (device copies): ``torch.save`` of it is a policy.pth,
        ``DevicePolicy(sd_on_cpu, ...)`` rebuilds the same policy"""
        p = self._flat()
        self._check(self.lib.adrp_ppo_params(self.h, p.data_ptr(), None, None, None, self._stream()), "adrp_ppo_params")
        return self._split(p)

    def snapshot(self, mode=None):
        """a new frozen ``DevicePolicy`` of the actor as it is now (its weights from ``state_dict()``, the learner
        policy's activation, its mode unless ``mode`` names another): later updates, which rewrite the learner
        policy in place, do not move it.  A self-play opponent for ``RosterRolloutCollector`` / ``simulate()``;
        the caller closes it."""
        from .policy import MODES, DevicePolicy
        sd = self.state_dict()
        if mode is None:
            mode = next(k for k, v in MODES.items() if v == self.policy.mode)
        return DevicePolicy({k: sd[k].cpu().numpy() for k in ACTOR_KEYS}, self.policy.activation, self.device.index, mode)

    def load_state_dict(self, sd):
        p = self._join(sd)
        self._check(self.lib.adrp_ppo_set_params(self.h, p.data_ptr(), None, None, -1, self._stream()), "adrp_ppo_set_params")
        torch.cuda.current_stream(self.device).synchronize()      # p may be freed after the call

    def optimizer_state_dict(self):
        """Adam's state: {"exp_avg": {key: tensor}, "exp_avg_sq": {key: tensor}, "step": int}"""
        m, v = self._flat(), self._flat()
        t = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._check(self.lib.adrp_ppo_params(self.h, None, m.data_ptr(), v.data_ptr(), t.data_ptr(), self._stream()),
                    "adrp_ppo_params")
        return {"exp_avg": self._split(m), "exp_avg_sq": self._split(v), "step": int(t.item())}

    def load_optimizer_state_dict(self, osd):
        m, v = self._join(osd["exp_avg"]), self._join(osd["exp_avg_sq"])
        self._check(self.lib.adrp_ppo_set_params(self.h, None, m.data_ptr(), v.data_ptr(), int(osd["step"]), self._stream()),
                    "adrp_ppo_set_params")
        torch.cuda.current_stream(self.device).synchronize()

    def gradients(self):
        """{SB3 key: tensor}: the raw (pre-clip) gradients of the last update"""
        gflat = self._flat()
        self._check(self.lib.adrp_ppo_gradients(self.h, gflat.data_ptr(), self._stream()), "adrp_ppo_gradients")
        return self._split(gflat)

    def set_target_kl(self, target_kl):
        """None: no early stop (the state of a new learner); otherwise SB3's ``target_kl`` for the updates issued from
        now on (a latch that has tripped holds until the next ``train_begin``, which ``train`` calls)"""
        if target_kl is not None:
            target_kl = float(target_kl)
            if not target_kl >= 0.0:
                raise ValueError("target_kl must be None or a number >= 0")
        if target_kl is not None or hasattr(self.lib, "adrp_ppo_set_target_kl"):
            self._check(self.lib.adrp_ppo_set_target_kl(self.h, -1.0 if target_kl is None else target_kl), "adrp_ppo_set_target_kl")
        self.target_kl = target_kl

    def set_rates(self, learning_rate, clip_range, clip_range_vf=None):
        """the learning rate and clip ranges of the updates issued from now on (floats; a captured graph keeps the
        values it was captured with)"""
        vf = -1.0 if clip_range_vf is None else float(clip_range_vf)
        if clip_range_vf is not None and not vf >= 0:
            raise ValueError("clip_range_vf must not be negative")
        self._check(self.lib.adrp_ppo_set_rates(self.h, float(learning_rate), float(clip_range), vf), "adrp_ppo_set_rates")
        self.cfg.learning_rate, self.cfg.clip_range, self.cfg.clip_range_vf = float(learning_rate), float(clip_range), vf

    def train_begin(self):
        """clears the target_kl latch on the current stream (``train`` calls it; capturable)"""
        self._check(self.lib.adrp_ppo_train_begin(self.h, self._stream()), "adrp_ppo_train_begin")

    def read_stop_state(self):
        """copies the latch into ``stop_state`` (device int32 [2]: tripped, optimizer steps applied since
        ``train_begin``) on the current stream and returns it; no host read"""
        self._check(self.lib.adrp_ppo_stop_state(self.h, self.stop_state.data_ptr(), self._stream()), "adrp_ppo_stop_state")
        return self.stop_state

    def stop_info(self):
        """the one deliberate host read: {"stopped", "updates", "epoch", "minibatch"} of the last ``train``.  When it
        stopped, ``epoch`` / ``minibatch`` are those of the minibatch whose KL tripped the stop (its step was not
        applied), else None"""
        with torch.cuda.device(self.device):
            stopped, updates = self.read_stop_state().cpu().tolist()
        at = divmod(updates, self._nmb) if stopped and self._nmb else (None, None)
        return {"stopped": bool(stopped), "updates": updates, "epoch": at[0], "minibatch": at[1]}

    def update(self, obs, actions, old_values, old_log_prob, advantages, returns, idx, stats=None):
        """one minibatch: rows ``idx`` (int64 device tensor) of the flattened buffers obs [R, D],
        actions [R, A], old_values / old_log_prob / advantages / returns [R] -> stats [5] (device:
        policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction)"""
        R = obs.shape[0]
        for t, n in ((obs, None), (actions, R * self.policy.act_dim), (old_values, R), (old_log_prob, R), (advantages, R),
                     (returns, R)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and (n is None or t.numel() == n)):
                raise ValueError("the buffers must be contiguous float32 device tensors of matching row count")
        if obs.dim() != 2 or obs.shape[1] < self.policy.in_dim:
            raise ValueError("obs must be [rows, D] with D >= the policy's in_dim")
        if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 1):
            raise ValueError("idx must be a contiguous int64 device tensor")
        stats = self._stats if stats is None else stats
        assert stats.is_cuda and stats.dtype == torch.float32 and stats.numel() == 5 and stats.is_contiguous()
        rc = self.lib.adrp_ppo_update(self.h, obs.data_ptr(), obs.shape[1], actions.data_ptr(), old_values.data_ptr(),
                                      old_log_prob.data_ptr(), advantages.data_ptr(), returns.data_ptr(), idx.data_ptr(),
                                      idx.numel(), stats.data_ptr(), self._stream())
        self._check(rc, "adrp_ppo_update")
        return stats

    def train(self, col, permutations=None, target_kl=None, progress_remaining=1.0):
        """``n_epochs`` passes over the collector's T x E samples, each a fresh random permutation cut
        into consecutive slices of ``batch_size`` (the last one shorter), as RolloutBuffer.get yields
        them.  ``permutations``: int64 [n_epochs, T E] to use instead of ``torch.randperm``.  Returns
        the statistics [n_epochs, n_minibatches, 5] (device tensor; nothing is read back).

        A collector with a ``valid`` attribute (``MultiAgentRolloutCollector``: [T, E] uint8, 0 for the samples
        of a drone whose agent episode is over) is trained on its valid rows only: each epoch permutes the
        n_valid flat indices of those rows (one ``torch.nonzero`` per call, the call's one host read), and
        ``permutations`` is then int64 [n_epochs, n_valid] of such indices.

        With a target set (``set_target_kl``; the ``target_kl`` keyword here is refused) the
        statistics are pre-filled with NaN: once a minibatch's approx_kl exceeds 1.5 target_kl its row is the last
        one written, its optimizer step and every later minibatch are skipped on the device (``stop_state``,
        ``stop_info()``); every launch is still issued and nothing is read back.  ``progress_remaining`` is what
        callable rates are evaluated at, once, before the first update."""
        if target_kl is not None:
            raise ValueError(_NO_KEYWORD)
        if self._scheduled:
            self.set_rates(_rate(self.learning_rate, progress_remaining), _rate(self.clip_range, progress_remaining),
                           None if self.clip_range_vf is None else _rate(self.clip_range_vf, progress_remaining))
        n = col.T * col.E
        flat = (col.obs.view(n, -1), col.actions.view(n, -1), col.values.view(n), col.log_probs.view(n),
                col.advantages.view(n), col.returns.view(n))
        # the index pool: every row, or the valid ones (no index of another row reaches ``update``)
        rows, pool, what = None, n, str(n)
        if getattr(col, "valid", None) is not None:
            valid = col.valid.view(n) != 0
            rows = torch.nonzero(valid).view(-1)              # int64, ascending; the host learns n_valid here
            pool, what = rows.numel(), f"n_valid = {rows.numel()}"
            if pool == 0:
                raise ValueError("the rollout holds no valid sample")
        if permutations is not None:
            permutations = permutations.to(device=self.device, dtype=torch.int64).contiguous()
            if tuple(permutations.shape) != (self.n_epochs, pool):
                raise ValueError(f"permutations must be [n_epochs, {what}]")
            if rows is not None:
                inside = (permutations >= 0) & (permutations < n)
                if not bool((inside & valid[permutations.clamp(0, n - 1)]).all()):
                    raise ValueError("permutations holds the index of an invalid row")
        nmb = (pool + self.batch_size - 1) // self.batch_size
        if self.target_kl is None:
            stats = torch.zeros((self.n_epochs, nmb, 5), dtype=torch.float32, device=self.device)
        else:       # the minibatches behind a stop write nothing
            stats = torch.full((self.n_epochs, nmb, 5), float("nan"), dtype=torch.float32, device=self.device)
        self._nmb = nmb
        with torch.cuda.device(self.device):
            if hasattr(self.lib, "adrp_ppo_train_begin"):     # (an A/B run on the parent commit's build has no latch)
                self.train_begin()
            for e in range(self.n_epochs):
                if permutations is not None:
                    perm = permutations[e]
                else:
                    perm = torch.randperm(pool, device=self.device, generator=self._gen)
                    if rows is not None:
                        perm = rows[perm]
                for k, s in enumerate(range(0, pool, self.batch_size)):
                    self.update(*flat, perm[s:s + self.batch_size], stats=stats[e, k])
            if hasattr(self.lib, "adrp_ppo_stop_state"):
                self.read_stop_state()
        return stats

    def close(self):
        if getattr(self, "h", None):
            self.lib.adrp_ppo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
