"""``ppo_reference.train_loop`` with stable_baselines3 2.3.2 ``PPO.train()``'s ``target_kl`` stop, restated from its
published code, and the cases the target_kl tests run (tests/test_ppo_target_kl_abi.py on the CPU,
tests/test_ppo_target_kl_gpu.py on the device).  CPU only.

SB3, inside the minibatch loop, after the loss and before ``optimizer.zero_grad()``:
    approx_kl_div = mean((exp(log_ratio) - 1) - log_ratio)             (no_grad, the policy's dtype)
    approx_kl_divs.append(approx_kl_div)
    if target_kl is not None and approx_kl_div > 1.5 * target_kl: continue_training = False; break
and after the minibatch loop ``if not continue_training: break``.  The comparison is made in float64: the
statistic widened, ``1.5 * target_kl`` a double product; a NaN compares false.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests import ppo_reference as R


def train_loop_kl(weights, buffers_np, perms, batch_size, cfg, relu, dtype, target_kl=None):
    """-> (final {key: tensor}, [approx_kl of every minibatch that was evaluated, as a float], trip index or
    None): the flat index of the minibatch whose KL tripped the stop (its optimizer step not applied, its KL the
    last of the list)"""
    p = R.to_params(weights, dtype)
    opt = torch.optim.Adam([p[k] for k in R.KEYS], lr=cfg.learning_rate, eps=1e-5)
    buf = tuple(torch.tensor(np.asarray(b), dtype=dtype) for b in buffers_np)
    kls, trip = [], None
    for perm in perms:
        perm = torch.as_tensor(perm, dtype=torch.int64)
        for s in range(0, len(perm), batch_size):
            j = perm[s:s + batch_size]
            total, stats, _ = R.loss(p, tuple(b[j] for b in buf), cfg, relu)
            kl = float(stats["approx_kl"])                      # the dtype's value, widened
            kls.append(kl)
            if target_kl is not None and kl > 1.5 * float(target_kl):
                trip = len(kls) - 1
                break
            opt.zero_grad()
            total.backward()
            torch.nn.utils.clip_grad_norm_([p[k] for k in R.KEYS], cfg.max_grad_norm)
            opt.step()
        if trip is not None:
            break
    return {k: p[k].detach() for k in R.KEYS}, kls, trip


# in, h1, h2, act, activation, rows, batch, epochs | learning rate, seed, the trip index k* the case aims at
CASES = [
    SimpleNamespace(shape=(5, 16, 32, 3), activation="tanh", rows=96, batch=32, epochs=4, lr=3e-3, seed=23, k=6),
    SimpleNamespace(shape=(144, 64, 64, 8), activation="tanh", rows=128, batch=64, epochs=3, lr=3e-3, seed=11, k=3),
    SimpleNamespace(shape=(49, 128, 128, 4), activation="relu", rows=64, batch=32, epochs=2, lr=3e-3, seed=20, k=2),
]

_cache = {}


def case(i):
    """the i-th case, computed once and shared (do not modify): weights, buffers (lp_noise = 0: the first minibatch's
    KL is 0), the explicit permutations, cfg, the float64 and float32 KL sequences of the run without a stop, k*,
    target_kl with 1.5 target_kl half way between max(KL[:k*]) and KL[k*], and the two margins"""
    if i not in _cache:
        c = CASES[i]
        relu = c.activation == "relu"
        w = R.make_weights(*c.shape, c.seed)
        buf = R.make_buffers(w, c.rows, relu, c.seed + 1, lp_noise=0)
        perms = np.stack([np.random.default_rng(c.seed + 2 + e).permutation(c.rows) for e in range(c.epochs)])
        cfg = R.config(learning_rate=c.lr)
        _, kl64, none64 = train_loop_kl(w, buf, perms, c.batch, cfg, relu, torch.float64)
        _, kl32, none32 = train_loop_kl(w, buf, perms, c.batch, cfg, relu, torch.float32)
        assert none64 is None and none32 is None
        nmb = math.ceil(c.rows / c.batch)
        below, at = max(kl64[:c.k]), kl64[c.k]
        thr = 0.5 * (below + at)
        _cache[i] = SimpleNamespace(
            c=c, relu=relu, w=w, buf=buf, perms=perms, cfg=cfg, kl64=kl64, kl32=kl32, nmb=nmb, n=nmb * c.epochs, k=c.k,
            target_kl=thr / 1.5, thr=thr, below=below, at=at,
            # the float32-vs-float64 deviation of the statistic in the reference's own two runs, up to the trip
            dev=max(abs(a - b) for a, b in zip(kl32[:c.k + 1], kl64[:c.k + 1])))
    return _cache[i]
