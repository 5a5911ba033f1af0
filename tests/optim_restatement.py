"""What the optimiser tests share (test_optim_host.py, test_optim_gpu.py): the chunk plan of csrc/vlg_optim.hip restated in Python, the case
table, the inputs, the float64 torch oracle and the derived bounds.

Bounds (derived, not tuned), after K <= 5 updates:
  |p - p64| <= K (2^-22 |p64| + 2^-16 lr lr_mult)   the master is rounded once per update (2^-24 relative; 4x margin); the update is at most a
                                                    few lr and its float32 evaluation carries about ten roundings plus the norm's error,
                                                    below 2^-19 relative (2x margin)
  m, v within K 2^-20 relative (+ 1e-30)            a RELATIVE bound holds in float32 only where nothing cancels, so the inputs are drawn so
                                                    that nothing does: every element keeps ONE sign in its parameter and in all its gradients
                                                    (m, and g + weight_decay p, are then sums of same-signed terms)
  norm within 2^-20, coef and lr within 2^-22 relative
A fourth regime, "mixed", draws an independent sign for the parameter and for every gradient: p is held to the same absolute bound, m and v to
absolute bounds (`absolute_scale`).
test_optim_host.py asserts that float32 torch.optim.Adam on the CPU meets all of them on these very inputs, before any kernel is compared.
"""
import functools

import torch

CHUNK, CAPACITY, NORM_GRID, GRID, SCALAR_BYTES = 4096, 128, 512, 2048, 256
SIZES = (1, 2, 3, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
OFFSETS = (0, 1, 3, 5)     # element offsets of the views: 16-byte aligned (0) and aligned to the element only
LR, BETAS, EPS, GAMMA, MAX_NORM, K = 1e-3, (0.9, 0.999), 1e-12, 0.75 ** (1 / 2000), 5.0, 3
GROUPS = [{"pattern": r"b\.", "lr_mult": 0.5, "weight_decay": 0.01}, {"pattern": r"a\.", "lr_mult": 1.0, "weight_decay": 0.0}]
REGIMES = ("zero", "five", "forty", "mixed")
CAPTURED_ORDER = (0, 1, 2, 0, 1)     # the captured-update test: two warm-up updates, then three replays -- five updates in all


# ---- the chunk plan --------------------------------------------------------------------------------------------------------------------
def chunk_plan(numels):
    """[(launch, tensor, offset, length)] in chunk order: tensor by tensor, CHUNK elements each, CAPACITY tensors per launch."""
    plan = []
    for i, n in enumerate(numels):
        plan += [(i // CAPACITY, i, lo, min(CHUNK, n - lo)) for lo in range(0, n, CHUNK)]
    return plan


def launches(numels):
    """Per launch: (chunks, squared-sum grid = slots, update grid)."""
    out = []
    for first in range(0, len(numels), CAPACITY):
        chunks = sum(-(-n // CHUNK) for n in numels[first:first + CAPACITY])
        out.append((chunks, min(chunks, NORM_GRID), min(chunks, GRID)))
    return out


def workspace_bytes(numels):
    if not numels:
        return 0
    return (SCALAR_BYTES + 8 * sum(s for _, s, _ in launches(numels)) + 255) // 256 * 256


# ---- the case table --------------------------------------------------------------------------------------------------------------------
def case_table():
    """CAPACITY + 2 tensors: the sizes around the chunk, then small fillers.  Per tensor: name (group a / b), numel, whether the parameter is
    bf16 (has a shadow), the gradient's dtype, and the element offset of each of its five arrays inside its sentinel-filled buffer."""
    sizes = list(SIZES) + [5 + (i % 20) for i in range(CAPACITY + 2 - len(SIZES))]
    rows = []
    for i, n in enumerate(sizes):
        rows.append(dict(name=f"{'b' if i % 3 == 0 else 'a'}.t{i:03d}", numel=n, shadow=i % 2 == 0,
                         grad_dtype=torch.bfloat16 if (i >> 1) & 1 else torch.float32,
                         off=dict(p=OFFSETS[i % 4], m=OFFSETS[(i + 1) % 4], v=OFFSETS[(i // 2) % 4], s=OFFSETS[(i // 3) % 4], g=OFFSETS[(i + i // 4) % 4])))
    return rows


def options(rows):
    from vlgae_amd import optim
    return optim.resolve_groups([r["name"] for r in rows], GROUPS)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def draw(regime):
    """(signs, p0, grads[K]) on the CPU, per tensor of the case table, in the dtypes the kernel gets (the parameter bf16 where it has a
    shadow).  |p| in [2^-6, 2], |g| in [2^-8, 4] or exactly 0; one sign per element (see the module docstring)."""
    g = torch.Generator().manual_seed(20240 + REGIMES.index(regime))
    rows = case_table()
    signs, p0, grads = [], [], [[] for _ in range(K)]
    for r in rows:
        n = r["numel"]
        s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        p = s * torch.exp2(-6 + 7 * torch.rand(n, generator=g))
        signs.append(s)
        p0.append(p.to(torch.bfloat16) if r["shadow"] else p)
        for k in range(K):
            mag = torch.exp2(-8 + 10 * torch.rand(n, generator=g) ** 16)
            keep = torch.rand(n, generator=g) >= 0.1
            if regime == "mixed":   # an independent sign per draw: m changes sign, g + weight_decay p can cancel (absolute bounds only)
                sk = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
                x = torch.where(keep, sk * mag, torch.zeros(n))
            else:
                x = torch.where(keep, s * mag, torch.zeros(n)) if regime == "forty" else torch.zeros(n)
            grads[k].append(x.to(r["grad_dtype"]))
    if regime == "five":   # two elements, 3 and 4, at other places in every update: norm exactly 5
        for k in range(K):
            a, b = 6 + k, 9 - k                                    # the big tensors: both dtypes, both groups
            grads[k][a][10 + k] = 3.0 * signs[a][10 + k]
            grads[k][b][rows[b]["numel"] - 1 - k] = 4.0 * signs[b][rows[b]["numel"] - 1 - k]
    return signs, p0, grads


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def oracle(p0, grads, opts, dtype=torch.float64, max_norm=MAX_NORM, lr=LR, lr_scale_before=None):
    """clip_grad_norm_, torch.optim.Adam(foreach=False).step(), ExponentialLR.step(), once per entry of `grads`, on the CPU in `dtype`,
    from the masters cast up.  opts: [(lr_mult, weight_decay)] per tensor.  lr_scale_before: {k: factor} multiplies the learning rate
    before update k (0-based) -- what overwriting the optimiser's base lr by lr * factor means.
    Returns dict(p, m, v: lists per tensor; norm, coef, lr: lists per update (lr: the base rate used, without lr_mult))."""
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in p0]
    groups = [dict(params=[p], lr=lr * lm, weight_decay=wd) for p, (lm, wd) in zip(params, opts)]
    opt = torch.optim.Adam(groups, lr=lr, betas=BETAS, eps=EPS, foreach=False)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=GAMMA)
    scale = 1.0
    norms, coefs, lrs = [], [], []
    for k, gs in enumerate(grads):
        if lr_scale_before and k in lr_scale_before:
            scale *= lr_scale_before[k]
            for grp in opt.param_groups:
                grp["lr"] *= lr_scale_before[k]
        for p, x in zip(params, gs):
            p.grad = x.to(dtype).clone()
        if max_norm is None:
            norm = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params))
            coefs.append(1.0)
        else:
            norm = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
            coefs.append(min(1.0, max_norm / (float(norm) + 1e-6)))
        norms.append(float(norm))
        lrs.append(lr * scale * GAMMA ** k)
        opt.step()
        sched.step()
    return dict(p=[p.detach() for p in params], m=[opt.state[p]["exp_avg"] for p in params], v=[opt.state[p]["exp_avg_sq"] for p in params],
                norm=norms, coef=coefs, lr=lrs)


@functools.lru_cache(maxsize=None)
def oracle64(regime, clip=True):
    """The float64 oracle of a regime of the case table, computed once and shared (treat as read-only)."""
    _, p0, grads = draw(regime)
    opts = list(options(case_table()).values())
    return oracle(p0, grads, opts, torch.float64, MAX_NORM if clip else None)


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------
def absolute_scale(p0, grads, opts):
    """Per tensor, A >= |coef g + weight_decay p| of every update, elementwise: max_k |g_k| + weight_decay (|p0| + 0.01) (coef <= 1, and p
    moves by a few lr).  With signs that change, m and v are sums whose terms cancel: their float32 error is relative to the TERMS, so the
    bounds of the "mixed" regime are K 2^-20 A for m and K 2^-20 A^2 for v (the relative bounds with the largest term in place of the sum)."""
    return [torch.stack([g[i].double().abs() for g in grads]).max(0).values + wd * (p0[i].double().abs() + 0.01) for i, (_, wd) in enumerate(opts)]


def check_against(ref, got, opts, n_updates, lr=LR, what="", scale=None):
    """got / ref: dict(p, m, v lists; norm, coef, lr lists) -- assert the bounds of the module docstring (ref in float64).  scale: the
    `absolute_scale` of the inputs -- m and v are then held to the absolute bounds described there."""
    for i, (lm, _) in enumerate(opts):
        p64, m64, v64 = ref["p"][i].double(), ref["m"][i].double(), ref["v"][i].double()
        bound = n_updates * (2.0 ** -22 * p64.abs() + 2.0 ** -16 * lr * lm)
        err = (got["p"][i].double().cpu() - p64).abs()
        assert bool((err <= bound).all()), (what, "p", i, float((err / bound).max()))
        for name, x64 in (("m", m64), ("v", v64)):
            if name in got:
                err = (got[name][i].double().cpu() - x64).abs()
                size = x64.abs() if scale is None else (scale[i] if name == "m" else scale[i] ** 2)
                lim = n_updates * 2.0 ** -20 * size + 1e-30
                assert bool((err <= lim).all()), (what, name, i, float((err / lim).max()))
    for k in range(len(ref["norm"])):
        for name, rel in (("norm", 2.0 ** -20), ("coef", 2.0 ** -22), ("lr", 2.0 ** -22)):
            if name in got:
                assert abs(got[name][k] - ref[name][k]) <= rel * abs(ref[name][k]), (what, name, k, got[name][k], ref[name][k])

