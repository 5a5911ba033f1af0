"""GPU: expectations under DependencyCRF on an MI355X -- vlg_deptree_expect at every chart placement and boundary in f32 and bf16, the
four methods (expected_score / tree_entropy / tree_cross_entropy / tree_kl) and all their gradients against the reference's fixtures and
the float64 restatement, structural identities that need no oracle, forbidden arcs and bad lengths, and capture into a HIP graph.

Every case is B = 3 ragged sentences (lengths N - 1, 1, (N - 1) // 2).  Tolerances (tests/expect_restatement.py) are against the
float64 restatement: the floor of each output, or 6 x the error of the float32 restatement on the same inputs where that is larger;
every test prints its error / bound ratios.

Measured on an MI355X, largest error / bound: logZ 0.006, ev 0.002, mu 0.23, hv 0.28 (both at N = 255, workspace placement); the four
methods' values 0.006, their gradients 0.073 (d tree_entropy / d arc_p at the first workspace N); the structural identities 0.11.
"""
import functools
import os

import numpy as np
import pytest
import torch

import expect_restatement as E
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
GUARD = 256   # floats of NaN on either side of every output


@pytest.fixture(scope="module")
def dev():
    from vlgae_amd.build import build_library
    build_library()
    return torch.device("cuda")


def ragged(N):
    return np.array([N - 1, 1, max(1, (N - 1) // 2)], np.int64)


def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def placement_ns():
    """{2, 3, 6, 41, 42, 255} and {b - 1, b} for every N at which either op changes placement: from the restated layout, which must
    agree with the library's size query about where each op first needs a workspace."""
    from vlgae_amd import _C
    q = _C.lib().vlg_workspace_bytes
    bs = E.boundaries()
    for grad, op in ((False, _C.OP_DEPTREE_EXPECT), (True, _C.OP_DEPTREE_EXPECT_GRAD)):
        first = next(N for N in range(2, 256) if q(op, 1, N, 0) > 0)
        assert first in bs and E.plan(first, grad)[2] > 0 == E.plan(first - 1, grad)[2]
        assert all(q(op, 1, N, 0) == E.plan(N, grad)[2] for N in range(2, 256))
    return sorted({2, 3, 6, 41, 42, 255} | set(bs) | {b - 1 for b in bs})


PLACEMENT_NS = sorted({2, 3, 6, 41, 42, 255} | set(E.boundaries()) | {b - 1 for b in E.boundaries()})


@functools.lru_cache(maxsize=None)
def batch(N, bf16, seed=0):
    "(arc, v, lengths, (r64, r32)): one float64 and one float32 restatement per (N, dtype), shared"
    rng = np.random.default_rng(500 + N + seed)
    arc = rng.standard_normal((3, N, N)).astype(np.float32)
    v = (0.5 * rng.standard_normal((3, N, N))).astype(np.float32)
    if bf16:
        arc, v = _bf16_round(arc), _bf16_round(v)
    ln = ragged(N)
    return arc, v, ln, (E.dual_batch(arc, ln, v, None, np.float64), E.dual_batch(arc, ln, v, None, np.float32))


def run_abi(dev, arc, v, v_sub, lengths, grad=True, bf16=False, want=(True, True)):
    """vlg_deptree_expect called directly: outputs inside NaN guard bands, the workspace prefilled with NaN.  Returns numpy
    (logZ, ev, mu, hv) after checking that the bands are untouched."""
    from vlgae_amd import _C
    B, N = arc.shape[:2]
    dt = torch.bfloat16 if bf16 else torch.float32
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt).contiguous()
    arc_t, v_t, s_t = t(arc), t(v), t(v_sub)
    ln = torch.from_numpy(np.ascontiguousarray(lengths, np.int64)).to(dev)
    sizes = [B, B] + ([B * N * N if w else 0 for w in want] if grad else [0, 0])
    offs, total = [], GUARD
    for s in sizes:
        offs.append(total)
        total += ((s + 63) & ~63) + GUARD
    flat = torch.full((total,), float("nan"), device=dev)
    views = [flat[o:o + s] if s else None for o, s in zip(offs, sizes)]
    op = _C.OP_DEPTREE_EXPECT_GRAD if grad and any(want) else _C.OP_DEPTREE_EXPECT
    nb = _C.lib().vlg_workspace_bytes(op, B, N, 0)
    ws = torch.full((nb // 4 + 1,), float("nan"), device=dev) if nb else None
    code = (_C.BF16 if bf16 else _C.F32)
    _C.check(_C.lib().vlg_deptree_expect(_C.ptr(arc_t), _C.ptr(v_t), _C.ptr(s_t), _C.ptr(ln), B, N, code, code, *[_C.ptr(x) for x in views],
                                         _C.ptr(ws), nb, _C.stream_of(arc_t)), "deptree_expect")
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    keep = np.zeros(total, bool)
    for o, s in zip(offs, sizes):
        keep[o:o + s] = True
    assert np.isnan(host[~keep]).all(), "a guard band was written"
    out = [None if not s else host[o:o + s] for o, s in zip(offs, sizes)]
    return out[0], out[1], None if out[2] is None else out[2].reshape(B, N, N), None if out[3] is None else out[3].reshape(B, N, N)


def report(tag, r):
    print(f"{tag}: error / bound " + " ".join(f"{k} {x:.3f}" for k, x in sorted(r.items())))
    assert all(x <= 1.0 for x in r.values()), (tag, r)


# ---- 1. every placement boundary ------------------------------------------------------------------------------------------------------
def _grad_ws_n():
    "the first N at which the inside-outside image keeps charts in the workspace"
    return next(N for N in range(2, 256) if E.plan(N, True)[2] > 0)


def test_boundaries_come_from_the_query(dev):
    assert placement_ns() == PLACEMENT_NS


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("N", PLACEMENT_NS)
def test_every_placement(dev, N, bf16):
    arc, v, ln, refs = batch(N, bf16)
    got = run_abi(dev, arc, v, None, ln, bf16=bf16)
    report(f"expect N={N} {'bf16' if bf16 else 'f32'} mode {E.plan(N, True)[0]}", E.ratios(got, arc, ln, v, refs=refs))
    fw = run_abi(dev, arc, v, None, ln, grad=False, bf16=bf16)
    report(f"expect forward only N={N} mode {E.plan(N, False)[0]}", E.ratios(fw, arc, ln, v, refs=refs))
    assert fw[2] is None and fw[3] is None
    assert np.array_equal(fw[0], got[0]) and np.array_equal(fw[1], got[1])   # one value pass in both images: the same bits (tree_kl relies on it)
    if N in (6, _grad_ws_n()):   # each optional output on its own: the others unchanged
        only_mu, only_hv = run_abi(dev, arc, v, None, ln, want=(True, False)), run_abi(dev, arc, v, None, ln, want=(False, True))
        assert np.array_equal(only_mu[2], got[2]) and np.array_equal(only_hv[3], got[3]) and np.array_equal(only_hv[0], got[0])


# ---- 2. the four methods and all their gradients --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def method_case(name):
    """Inputs and float64 references {quantity: (value [B], {input: gradient [B,N,N]})} plus the float32 restatement's versions: from a
    fixture of the reference, or (name = N) from the restatement."""
    if isinstance(name, str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        p, q, c, ln = z["arc_p"], z["arc_q"], z["cost"], z["lengths"]
    else:
        rng = np.random.default_rng(name)
        p, q, c = (rng.standard_normal((3, name, name)).astype(np.float32).astype(np.float64) for _ in range(3))   # float32 values
        ln = ragged(name)

    def quantities(dtype):
        lzq, _, muq, _ = E.dual_batch(q, ln, None, None, dtype)
        lz, ev, mu, hv = E.dual_batch(p, ln, p, None, dtype)
        out = {"entropy": (lz - ev, {"arc_p": -hv})}
        lz, ev, mu, hv = E.dual_batch(p, ln, q, None, dtype)
        out["cross_entropy"] = (lzq - ev, {"arc_p": -hv, "arc_q": muq - mu})
        lz, ev, mu, hv = E.dual_batch(p, ln, q, p, dtype)
        out["kl"] = (lzq - lz - ev, {"arc_p": -hv, "arc_q": muq - mu})
        lz, ev, mu, hv = E.dual_batch(p, ln, c, None, dtype)
        out["risk"] = (ev, {"arc_p": hv, "cost": mu})
        return out

    r64, r32 = quantities(np.float64), quantities(np.float32)
    if isinstance(name, str):   # the reference's own numbers are the reference where there is a fixture
        for k in r64:
            assert np.abs(r64[k][0] - z[k]).max() <= 1e-10 * max(1.0, np.abs(z[k]).max())
            r64[k] = (z[k], {i: z[f"g_{k}_{i}"] for i in r64[k][1]})
    lz_p, _, mu_p, _ = E.dual_batch(p, ln)
    lz_q = E.dual_batch(q, ln)[0]
    scales = {"entropy": (lz_p, p), "cross_entropy": (np.maximum(np.abs(lz_p), np.abs(lz_q)), q),
              "kl": (np.maximum(np.abs(lz_p), np.abs(lz_q)), q - p), "risk": (lz_p, c)}
    vb = {k: [max(2e-5 * max(1.0, float(np.abs(s[0][b])), float((np.abs(mu_p[b]) * np.abs(E.direction(p, ln, s[1])[b])).sum())),
                  6.0 * abs(float(r32[k][0][b]) - float(r64[k][0][b]))) for b in range(len(ln))] for k, s in scales.items()}
    return p, q, c, ln, r64, r32, vb


@pytest.mark.parametrize("name", ("expect_B3_N6_s0", "expect_B4_N12_s1", "expect_B2_N41_s2", "ws"))
@pytest.mark.parametrize("upstream", ("weights", "sum"))
def test_methods_and_gradients(dev, name, upstream):
    from vlgae_amd.torch_struct import DependencyCRF
    key = _grad_ws_n() if name == "ws" else name
    p, q, c, ln, r64, r32, vb = method_case(key)
    B = len(ln)
    f64 = isinstance(key, str)                      # the fixtures go in as float64 tensors, the restatement case as float32
    dt = torch.float64 if f64 else torch.float32
    wts = np.linspace(-1.5, 2.0, B) if upstream == "weights" else np.ones(B)
    lengths = torch.from_numpy(ln).to(dev)
    worst = {}
    for k in ("entropy", "cross_entropy", "kl", "risk"):
        tp, tq, tc = (torch.tensor(a, dtype=dt, device=dev, requires_grad=True) for a in (p, q, c))
        dp, dq = DependencyCRF(tp, lengths), DependencyCRF(tq, lengths)
        val = {"entropy": dp.tree_entropy, "cross_entropy": lambda: dp.tree_cross_entropy(dq), "kl": lambda: dp.tree_kl(dq),
               "risk": lambda: dp.expected_score(tc)}[k]()
        assert val.shape == (B,) and val.dtype == dt
        (val.sum() if upstream == "sum" else (val * torch.tensor(wts, dtype=dt, device=dev)).sum()).backward()
        got = val.detach().cpu().numpy().astype(np.float64)
        for b in range(B):
            worst[k] = max(worst.get(k, 0.0), abs(got[b] - r64[k][0][b]) / vb[k][b])
        for i, t in (("arc_p", tp), ("arc_q", tq), ("cost", tc)):
            if i not in r64[k][1]:
                assert t.grad is None
                continue
            g = t.grad.cpu().numpy().astype(np.float64)
            assert t.grad.dtype == dt and np.isfinite(g).all()
            for b in range(B):
                ref, e32 = r64[k][1][i][b], np.abs(r32[k][1][i][b] - r64[k][1][i][b]).max()
                bound = (E.mu_bound(e32) if (k, i) == ("risk", "cost") else E.grad_bound(ref, e32)) * abs(wts[b])
                err = np.abs(g[b] - wts[b] * ref).max()
                if bound == 0.0:
                    assert err == 0.0, (k, i, b)
                else:
                    worst[f"d{k}/d{i}"] = max(worst.get(f"d{k}/d{i}", 0.0), err / bound)
    report(f"methods {name} upstream={upstream}", worst)


def test_forward_without_gradients_and_lengths_none(dev):
    "no input wants a gradient: the inside-only image; lengths None = N - 1"
    from vlgae_amd.torch_struct import DependencyCRF
    arc, v, _, _ = batch(12, False)
    ln = np.full(3, 11, np.int64)
    ta, tv = torch.from_numpy(arc).to(dev), torch.from_numpy(v).to(dev)
    d = DependencyCRF(ta)
    r64, r32 = E.dual_batch(arc, ln, arc), E.dual_batch(arc, ln, arc, None, np.float32)
    H = d.tree_entropy().cpu().numpy().astype(np.float64)
    H64, H32 = r64[0] - r64[1], r32[0].astype(np.float64) - r32[1]
    report("entropy, no gradients", {"H": max(abs(H[b] - H64[b]) / E.value_bound(r64[0][b], r64[2][b], arc[b], abs(H32[b] - H64[b])) for b in range(3))})
    assert torch.equal(d.tree_kl(DependencyCRF(tv)), DependencyCRF(ta, torch.from_numpy(ln).to(dev)).tree_kl(DependencyCRF(tv)))


# ---- 3. structural checks (no oracle) -------------------------------------------------------------------------------------------------
STRUCT_NS = (6, 41, _grad_ws_n())


@pytest.mark.parametrize("N", STRUCT_NS)
def test_constant_direction_column_sums_and_symmetry(dev, N):
    """Each quantity is held to the hv bound of its sentence: 1e-4 of the largest |hv| (float64), or 6 x the same quantity's error in
    the float32 restatement where that is larger.  A length-1 sentence has hv = 0 and bound 0: exact."""
    arc, v, ln, refs = batch(N, False)
    worst = {}

    def hold(name, err, bound):
        if bound == 0.0:
            assert err == 0.0, (name, err)
        else:
            worst[name] = max(worst.get(name, 0.0), err / bound)

    # a constant direction: every tree has len arcs, <c, tree> is constant and nothing varies.  hv is linear in the direction and so is
    # its rounding error: with the exact result 0 the floor is that of this sentence's 0.5 randn direction, one of smaller norm
    floor = [1e-4 * np.abs(refs[0][3][b]).max() for b in range(3)]
    const = np.full_like(arc, 0.75)
    c32 = E.dual_batch(arc, ln, const, None, np.float32)
    lz, ev, mu, hv = run_abi(dev, arc, const, None, ln)
    for b in range(3):
        hold("ev = c len", abs(ev[b] - 0.75 * ln[b]), E.value_bound(refs[0][0][b], refs[0][2][b], const[b], abs(float(c32[1][b]) - 0.75 * ln[b])))
        hold("hv = 0", np.abs(hv[b]).max(), max(floor[b], 6.0 * np.abs(c32[3][b]).max()))
    lz, ev, mu, hv = run_abi(dev, arc, v, None, ln)
    rng = np.random.default_rng(N)
    u = (0.5 * rng.standard_normal(arc.shape)).astype(np.float32)
    hu = run_abi(dev, arc, u, None, ln)[3]
    u64, u32 = E.dual_batch(arc, ln, u), E.dual_batch(arc, ln, u, None, np.float32)
    dot = lambda a, h, b: float((a[b].astype(np.float64) * h[b].astype(np.float64)).sum())
    for b in range(3):
        # every word has one head, sum_h mu[h,c] = 1 whatever the potentials: the columns of hv sum to 0
        hold("column sums", np.abs(hv[b].astype(np.float64).sum(0)).max(),
             max(floor[b], 6.0 * np.abs(refs[1][3][b].astype(np.float64).sum(0)).max()))
        # the Hessian is symmetric: <u, Hv> = <v, Hu>
        hold("symmetry", abs(dot(u, hv, b) - dot(v, hu, b)),
             max(floor[b], 1e-4 * np.abs(u64[3][b]).max(), 6.0 * abs(dot(u, refs[1][3], b) - dot(v, u32[3], b))))
    report(f"structure N={N}", worst)


@pytest.mark.parametrize("N", STRUCT_NS + (255,))
def test_kl_of_a_distribution_with_itself_is_exactly_zero(dev, N):
    from vlgae_amd.torch_struct import DependencyCRF
    arc = torch.from_numpy(batch(N, False)[0]).to(dev)
    ln = torch.from_numpy(ragged(N)).to(dev)
    p, q = arc.clone().requires_grad_(True), arc.clone().requires_grad_(True)
    kl = DependencyCRF(p, ln).tree_kl(DependencyCRF(q, ln))
    (kl * torch.tensor([1.0, -2.0, 3.0], device=dev)).sum().backward()
    assert not kl.detach().any() and not p.grad.any() and not q.grad.any()
    assert not DependencyCRF(arc, ln).tree_kl(DependencyCRF(arc, ln)).any()          # the inside-only image too
    p = arc.clone().requires_grad_(True)                                             # a fixed q: inside-outside for p, inside only for q
    kl = DependencyCRF(p, ln).tree_kl(DependencyCRF(arc, ln))
    kl.sum().backward()
    assert not kl.detach().any() and not p.grad.any()


@pytest.mark.parametrize("N", STRUCT_NS)
def test_entropy_and_kl_are_nonnegative_and_length_one_is_exact(dev, N):
    from vlgae_amd.torch_struct import DependencyCRF
    arc, v, ln, refs = batch(N, False)
    ta, tv, tl = torch.from_numpy(arc).to(dev).requires_grad_(True), torch.from_numpy(v).to(dev), torch.from_numpy(ln).to(dev)
    H = DependencyCRF(ta, tl).tree_entropy()
    H.sum().backward()
    kl = DependencyCRF(ta.detach(), tl).tree_kl(DependencyCRF(tv, tl)).cpu().numpy()
    lz64, _, mu64, _ = E.dual_batch(arc, ln)
    for b in range(3):
        bound = 2e-5 * max(1.0, abs(lz64[b]), float((np.abs(mu64[b]) * np.abs(arc[b])).sum()), float((np.abs(mu64[b]) * np.abs(v[b] - arc[b])).sum()))
        assert H[b].item() >= -bound and kl[b] >= -bound
    assert H[1].item() == 0.0 and not ta.grad[1].any()              # one word: one tree


@pytest.mark.parametrize("N", (41, _grad_ws_n()))   # every chart in LDS | per-sentence workspace slices
def test_a_sentence_does_not_depend_on_its_batch(dev, N):
    arc, v, ln, _ = batch(N, False)
    base = run_abi(dev, arc, v, None, ln)
    rng = np.random.default_rng(9)
    other_arc, other_v = rng.standard_normal((5, N, N)).astype(np.float32), rng.standard_normal((5, N, N)).astype(np.float32)
    for b in range(3):
        other_arc[4 - b], other_v[4 - b] = arc[b], v[b]
    lengths = np.array([7, N - 1, ln[2], ln[1], ln[0]], np.int64)
    got = run_abi(dev, other_arc, other_v, None, lengths)
    for b in range(3):
        assert all(np.array_equal(x[4 - b], y[b]) for x, y in zip(got, base))


# ---- 4. forbidden arcs, bad lengths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (12, _grad_ws_n()))
def test_forbidden_arcs_and_bad_lengths(dev, N):
    rng = np.random.default_rng(40 + N)
    arc = rng.standard_normal((3, N, N)).astype(np.float32)
    v = (0.5 * rng.standard_normal((3, N, N))).astype(np.float32)
    forbid = rng.random((3, N, N)) < 0.2
    forbid[:, np.arange(N - 1), np.arange(1, N)] = False          # the chain 0 -> 1 -> 2 ... stays allowed: the support is not empty
    arc[forbid] = -np.inf
    v[forbid] = 1e30                                              # garbage where nothing may be read
    ln = ragged(N)
    got = run_abi(dev, arc, v, None, ln)
    report(f"forbidden arcs N={N}", E.ratios(got, arc, ln, v))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert not got[2][forbid].any() and not got[3][forbid].any()
    for bad in (0, N):
        lengths = np.array([ln[0], bad, ln[2]], np.int64)
        out = run_abi(dev, arc, v, None, lengths)
        assert np.isnan(out[0][1]) and np.isnan(out[1][1]) and not out[2][1].any() and not out[3][1].any()
        for b in (0, 2):                                          # the neighbours: unaffected, bit for bit
            assert all(np.array_equal(x[b], y[b]) for x, y in zip(out, got))
        fw = run_abi(dev, arc, v, None, lengths, grad=False)
        assert np.isnan(fw[0][1]) and np.isnan(fw[1][1]) and np.array_equal(fw[0][[0, 2]], got[0][[0, 2]])


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------------
def test_entropy_with_backward_replays_on_new_potentials(dev):
    """Launches per call, from the code (functional.py): entropy and expected score 1 (+ 1 vlg_scale_counts in backward); cross-entropy
    and KL 2 (+ 1 in-place subtraction when arc_q wants a gradient, + 1 vlg_scale_counts for the pair in backward)."""
    from vlgae_amd.torch_struct import DependencyCRF
    N = 41
    a0, a1 = (torch.from_numpy(batch(N, False, seed=s)[0]).to(dev) for s in (0, 1))
    ln = torch.from_numpy(ragged(N)).to(dev)
    w = torch.tensor([0.5, -1.0, 2.0], device=dev)

    def step(x):
        x.grad = None
        H = DependencyCRF(x, ln).tree_entropy()
        (H * w).sum().backward()
        return H.detach(), x.grad

    static = a0.clone().requires_grad_(True)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step(static)
    torch.cuda.current_stream(dev).wait_stream(side)
    static.grad = None
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        H_g, g_g = step(static)
    for new in (a1, a0):
        with torch.no_grad():
            static.copy_(new)
        gr.replay()
        H_e, g_e = step(new.clone().requires_grad_(True))
        assert torch.equal(H_g, H_e) and torch.equal(g_g, g_e)
