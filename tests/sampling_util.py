"""Shared checks for the seeded-sampling tests (test_sampling_ref.py on
ref_backend, test_gpu_sampling.py on the kernel). The judge of both is the
float64 oracle in ops/reference.py (``sample_scores`` / ``sample_candidates``);
``fn(logits, inv_t, top_k, seed, step) -> int64 (B,)`` is the code under test,
with top_k an int where 0 means all."""
from __future__ import annotations

import numpy as np
import torch

from midgpt_amd.ops import reference as ref

NEG = float("-inf")

# (V, B, temperature, top_k)
OPT_CASES = [(37, 64, 0.7, None), (37, 64, 0.7, 5), (520, 64, 1.0, 20),
             (2056, 64, 0.1, 1), (50304, 4, 0.8, 50)]

# (V, top_k, temperature, bound): Pearson chi-square against the fp64
# softmax over the candidates must stay below ``bound``, the 1 - 1e-6 quantile
# scipy.stats.chi2.isf(1e-6, df) at df = 36, 4 and 20.
CHI2_CASES = [(37, None, 1.0, 91.5), (37, 5, 0.7, 33.4), (520, 20, 0.8, 65.4)]
CHI2_ROWS, CHI2_STEPS = 4096, 8


def inv_t_of(temperature: float) -> float:
    """fp32(1 / T) as a Python float: what ops.sample_tokens hands a backend."""
    return float(np.float32(1.0 / temperature))


def bf16_logits(V, B, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(B, V, generator=g)).to(torch.bfloat16)


def check_optimal(tokens, logits, inv_t, top_k, seed, step):
    """Per-row optimality of ``tokens`` against the oracle. eps = 2^-20 *
    max(1, max |finite score64| of the row): about 4 fp32 roundings plus two
    logf of at most 2 ulp are at most 8 * 2^-24 relative, times 2 for FMA
    contraction. Returns (rows decided by more than 2 eps, rows)."""
    tok = tokens.cpu().numpy()
    s64 = ref.sample_scores(logits, inv_t, seed, step)
    cand = ref.sample_candidates(logits, top_k)
    B, V = s64.shape
    assert tok.shape == (B,) and tok.dtype == np.int64
    assert ((0 <= tok) & (tok < V)).all(), tok
    rows = np.arange(B)
    assert cand[rows, tok].all(), f"non-candidates drawn in rows {np.nonzero(~cand[rows, tok])[0]}"
    mag = np.where(np.isfinite(s64), np.abs(s64), 0.0).max(axis=1)
    eps = 2.0 ** -20 * np.maximum(1.0, mag)
    masked = np.where(cand, s64, NEG)
    order = np.sort(masked, axis=1)
    best = order[:, -1]
    second = order[:, -2] if V > 1 else np.full(B, NEG)
    got = s64[rows, tok]
    assert (got >= best - eps).all(), \
        f"score below the best by {np.max(best - got):.3e}, eps {eps.min():.3e}"
    decided = (best - second) > 2 * eps
    want = masked.argmax(axis=1)
    assert (tok[decided] == want[decided]).all(), \
        f"rows {np.nonzero(decided & (tok != want))[0]} differ from the oracle's argmax"
    return int(decided.sum()), B


def tie_row(V, k, seed):
    """V distinct bf16 values in [-1, 1] in random order, with 7 entries set
    to one value so that the k-th largest is one of them. Returns (row, the 7
    tied indices)."""
    rng = np.random.default_rng(seed)
    vals = np.arange(V, dtype=np.float32) * (2.0 ** -5)     # exact in bf16
    vals = vals - vals[V // 2]
    desc = vals[::-1].copy()                                  # rank r -> value
    r0 = max(0, min(k - 1, V - 7))
    desc[r0:r0 + 7] = desc[r0]
    perm = rng.permutation(V)                                 # rank r sits at index perm[r]
    row = np.empty(V, dtype=np.float32)
    row[perm] = desc
    return torch.from_numpy(row).to(torch.bfloat16), np.sort(perm[r0:r0 + 7])


def half_inf_row(V, seed):
    rng = np.random.default_rng(seed)
    row = torch.from_numpy(rng.standard_normal(V).astype(np.float32)).to(torch.bfloat16)
    row[torch.from_numpy(rng.permutation(V)[:V // 2])] = NEG
    return row


def check_candidate_sets(fn, V, place=lambda x: x):
    """The candidate-set cases for k in 1, 2, V-1, V, V+3, each row repeated
    256 times over 8 steps. ``place`` moves a CPU (B, V) bf16 tensor to where
    ``fn`` wants it."""
    R, STEPS = 256, 8
    for k in (1, 2, V - 1, V, V + 3):
        # 7 copies of the k-th value: all kept, each of them comes out
        row, tied = tie_row(V, k, seed=100 + k)
        lg = row[None].repeat(R, 1)
        cand = ref.sample_candidates(lg, k)
        n_cand = V if k >= V else max(0, min(k - 1, V - 7)) + 7
        assert cand[0, tied].all() and cand[0].sum() == n_cand, (k, cand[0].sum())
        seen = set()
        dev = place(lg)
        for step in range(STEPS):
            tok = fn(dev, 1.0, k, 11, step).cpu().numpy()
            assert cand[np.arange(R), tok].all(), (k, step)
            seen.update(tok.tolist())
        assert set(tied.tolist()) <= seen, (k, tied, sorted(seen))
        # half the row -inf: never drawn, whatever k
        row = half_inf_row(V, seed=200 + k)
        lg = row[None].repeat(R, 1)
        cand = ref.sample_candidates(lg, k) & np.isfinite(lg.float().numpy())
        dev = place(lg)
        for step in range(STEPS):
            tok = fn(dev, 1.0, k, 12, step).cpu().numpy()
            assert cand[np.arange(R), tok].all(), (k, step)
        # one finite value: always that index
        lg = torch.full((R, V), NEG, dtype=torch.bfloat16)
        lg[:, (5 * k) % V] = -2.5
        tok = fn(place(lg), 1.0, k, 13, 3).cpu()
        assert (tok == (5 * k) % V).all(), k


def chi2_logits(V, top_k, inv_t):
    """One row of 1.5 * randn bf16 logits for a chi-square case: the first
    seed for which every expected count is >= 5 (a property of the input
    alone; ``check_chi2`` asserts it)."""
    for seed in range(1000):
        row = bf16_logits(V, 1, 1.5, 7000 + seed)
        p, cand = _probs(row, inv_t, top_k)
        if (p[cand] * CHI2_ROWS * CHI2_STEPS).min() >= 5.0:
            return row
    raise AssertionError("no suitable logits")


def _probs(row, inv_t, top_k):
    cand = ref.sample_candidates(row, top_k)[0]
    z = row[0].double().numpy() * inv_t
    z = np.where(cand, z, NEG)
    p = np.exp(z - z.max())
    return p / p.sum(), cand


def check_chi2(fn, V, top_k, temperature, bound, place=lambda x: x):
    inv_t = inv_t_of(temperature)
    row = chi2_logits(V, top_k, inv_t)
    p, cand = _probs(row, inv_t, top_k)
    n = CHI2_ROWS * CHI2_STEPS
    expected = p[cand] * n
    assert expected.min() >= 5.0, expected.min()
    dev = place(row.repeat(CHI2_ROWS, 1))
    counts = np.zeros(V, dtype=np.int64)
    for step in range(CHI2_STEPS):
        tok = fn(dev, inv_t, top_k or 0, 2024, step).cpu().numpy()
        counts += np.bincount(tok, minlength=V)
    assert counts[~cand].sum() == 0, "draws outside the candidates"
    stat = float((((counts[cand] - expected) ** 2) / expected).sum())
    print(f"SAMPLING chi2 V{V} k{top_k} T{temperature}: stat={stat:.1f} "
          f"df={int(cand.sum()) - 1} bound={bound}")
    assert stat < bound, (stat, bound)
