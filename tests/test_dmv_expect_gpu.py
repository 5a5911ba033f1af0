"""GPU: expectations under DMV1o on an MI355X -- vlg_dmv1o_expect at every chart placement and boundary in f32 and bf16, the four
methods of DMV1oExpect (expected_score / tree_entropy / tree_cross_entropy / tree_kl) and all their gradients against the reference's fixtures and the
float64 restatement, structural identities that need no oracle, forbidden entries and bad lengths, batch independence, and capture
into a HIP graph.

Every case is B = 3 ragged sentences (lengths N - 1, 1, (N - 1) // 2) of root-merged potentials.  Tolerances
(tests/dmv_expect_restatement.py, the family's bounds of tests/expect_restatement.py) are against the float64 restatement: the floor of
each output, or 6 x the error of the float32 restatement on the same inputs where that is larger; every test prints its error / bound
ratios.

Measured on an MI355X, largest error / bound: logZ 0.008, ev 0.007, mu_dec 0.27, mu_att 0.25, hv_dec 0.22, hv_att 0.21 (the last four
at N = 255, workspace placement); the four methods' values 0.008, their gradients 0.22 (d tree_cross_entropy / d dec_q on the N = 12
fixture); the structural identities 0.067 (the STOP probabilities of a side sum to 1, N = 41).  mu_dec is held to
dmv_expect_restatement.count_ratio: its GO entries are expected numbers of children, not probabilities (against the plain 5e-5 floor
of mu_bound the GO count 10.4 of one head at N = 81 reached 0.99).
"""
import functools
import os

import numpy as np
import pytest
import torch

import dmv_expect_restatement as E
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("dmvexpect_B3_N6_s0", "dmvexpect_B4_N12_s1", "dmvexpect_B2_N41_s2")
GUARD = 256   # floats of NaN on either side of every output
PLACEMENT_NS = sorted({2, 3, 6, 41, 42, 255} | set(E.boundaries()) | {b - 1 for b in E.boundaries()})
WS_N = E.first_workspace_n(True)   # the first N at which the inside-outside image keeps charts in the workspace


@pytest.fixture(scope="module")
def dev():
    from vlgae_amd.build import build_library
    build_library()
    return torch.device("cuda")


def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def batch(N, bf16, seed=0):
    "(dec, attach, v, lengths, (r64, r32)): one float64 and one float32 restatement per (N, dtype), shared"
    dec, attach, v = E.case(N, 500 + N + seed)
    if bf16:
        dec, attach, v = _bf16_round(dec), _bf16_round(attach), (_bf16_round(v[0]), _bf16_round(v[1]))
    ln = E.ragged(N)
    return dec, attach, v, ln, (E.dual_batch(dec, attach, ln, v, None, np.float64), E.dual_batch(dec, attach, ln, v, None, np.float32))


def run_abi(dev, dec, attach, v, v_sub, lengths, grad=True, bf16=False, want=(True, True, True, True)):
    """vlg_dmv1o_expect called directly: outputs inside NaN guard bands, the workspace prefilled with NaN.  Returns numpy
    (logZ, ev, mu_dec, mu_att, hv_dec, hv_att) after checking that the bands are untouched."""
    from vlgae_amd import _C
    B, N = dec.shape[:2]
    dt = torch.bfloat16 if bf16 else torch.float32
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt).contiguous()
    dec_t, att_t = t(dec), t(attach)
    dirs = [t(a) for a in (*(v or (None, None)), *(v_sub or (None, None)))]
    ln = torch.from_numpy(np.ascontiguousarray(lengths, np.int64)).to(dev)
    shapes = [(B,), (B,), dec.shape, attach.shape, dec.shape, attach.shape]
    sizes = [B, B] + [int(np.prod(s)) if grad and w else 0 for s, w in zip(shapes[2:], want)]
    offs, total = [], GUARD
    for s in sizes:
        offs.append(total)
        total += ((s + 63) & ~63) + GUARD
    flat = torch.full((total,), float("nan"), device=dev)
    views = [flat[o:o + s] if s else None for o, s in zip(offs, sizes)]
    nb = _C.lib().vlg_dmv1o_expect_workspace(B, N, int(grad and any(want)))
    ws = torch.full((nb // 4 + 1,), float("nan"), device=dev) if nb else None
    code = _C.BF16 if bf16 else _C.F32
    _C.check(_C.lib().vlg_dmv1o_expect(_C.ptr(dec_t), _C.ptr(att_t), *[_C.ptr(x) for x in dirs], _C.ptr(ln), B, N, code, code,
                                       *[_C.ptr(x) for x in views], _C.ptr(ws), nb, _C.stream_of(dec_t)), "dmv1o_expect")
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    keep = np.zeros(total, bool)
    for o, s in zip(offs, sizes):
        keep[o:o + s] = True
    assert np.isnan(host[~keep]).all(), "a guard band was written"
    return tuple(None if not s else host[o:o + s].reshape(shp) for o, s, shp in zip(offs, sizes, shapes))


def report(tag, r):
    print(f"{tag}: error / bound " + " ".join(f"{k} {x:.3f}" for k, x in sorted(r.items())))
    assert all(x <= 1.0 for x in r.values()), (tag, r)


# ---- 1. every placement boundary ------------------------------------------------------------------------------------------------------
def test_boundaries_come_from_the_query(dev):
    "the restated layout agrees with the library's size query at every N, so PLACEMENT_NS holds both sides of every boundary"
    from vlgae_amd import _C
    q = _C.lib().vlg_dmv1o_expect_workspace
    for grad in (False, True):
        assert all(q(1, N, int(grad)) == E.plan(N, grad)[2] for N in range(2, 256))
        first = next(N for N in range(2, 256) if q(1, N, int(grad)) > 0)
        assert first in E.boundaries() and first == E.first_workspace_n(grad)
    assert all(b in PLACEMENT_NS and b - 1 in PLACEMENT_NS for b in E.boundaries()) and WS_N in PLACEMENT_NS


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("N", PLACEMENT_NS)
def test_every_placement(dev, N, bf16):
    dec, attach, v, ln, refs = batch(N, bf16)
    got = run_abi(dev, dec, attach, v, None, ln, bf16=bf16)
    report(f"dmv expect N={N} {'bf16' if bf16 else 'f32'} mode {E.plan(N, True)[0]}", E.ratios(got, dec, attach, ln, v, refs=refs))
    fw = run_abi(dev, dec, attach, v, None, ln, grad=False, bf16=bf16)
    report(f"dmv expect forward only N={N} mode {E.plan(N, False)[0]}", E.ratios(fw, dec, attach, ln, v, refs=refs))
    assert all(o is None for o in fw[2:])
    assert np.array_equal(fw[0], got[0]) and np.array_equal(fw[1], got[1])   # one value pass in both images: the same bits (tree_kl relies on it)
    if N in (6, WS_N):   # each optional output on its own: the others' bits unchanged
        for k in range(4):
            only = run_abi(dev, dec, attach, v, None, ln, bf16=bf16, want=tuple(i == k for i in range(4)))
            assert np.array_equal(only[2 + k], got[2 + k]) and np.array_equal(only[0], got[0]) and np.array_equal(only[1], got[1])
            assert all(only[2 + i] is None for i in range(4) if i != k)


# ---- 2. the four methods and all their gradients --------------------------------------------------------------------------------------
INPUTS = {"entropy": ("dec_p", "att_p"), "cross_entropy": ("dec_p", "att_p", "dec_q", "att_q"), "kl": ("dec_p", "att_p", "dec_q", "att_q"),
          "risk": ("dec_p", "att_p", "cost_dec", "cost_att")}


@functools.lru_cache(maxsize=None)
def method_case(name):
    """Inputs and float64 references {quantity: (value [B], {input: gradient})} plus the float32 restatement's versions: from a fixture
    of the reference, or (name = N) from the restatement."""
    if isinstance(name, str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        x = {k: z[k] for k in ("dec_p", "att_p", "dec_q", "att_q", "cost_dec", "cost_att")}
        ln = z["lengths"]
    else:
        dp, ap, c = E.case(name, name)
        dq, aq, _ = E.case(name, name + 1)
        x = {k: a.astype(np.float64) for k, a in zip(("dec_p", "att_p", "dec_q", "att_q", "cost_dec", "cost_att"), (dp, ap, dq, aq, *c))}
        ln = E.ragged(name)
    p, q, c = (x["dec_p"], x["att_p"]), (x["dec_q"], x["att_q"]), (x["cost_dec"], x["cost_att"])

    def quantities(dtype):
        lzq, _, mqd, mqa, _, _ = E.dual_batch(*q, ln, None, None, dtype)
        lz, ev, md, ma, hd, ha = E.dual_batch(*p, ln, p, None, dtype)
        out = {"entropy": (lz - ev, dict(dec_p=-hd, att_p=-ha))}
        lz, ev, md, ma, hd, ha = E.dual_batch(*p, ln, q, None, dtype)
        out["cross_entropy"] = (lzq - ev, dict(dec_p=-hd, att_p=-ha, dec_q=mqd - md, att_q=mqa - ma))
        lz, ev, md, ma, hd, ha = E.dual_batch(*p, ln, q, p, dtype)
        out["kl"] = (lzq - lz - ev, dict(dec_p=-hd, att_p=-ha, dec_q=mqd - md, att_q=mqa - ma))
        lz, ev, md, ma, hd, ha = E.dual_batch(*p, ln, c, None, dtype)
        out["risk"] = (ev, dict(dec_p=hd, att_p=ha, cost_dec=md, cost_att=ma))
        return out

    r64, r32 = quantities(np.float64), quantities(np.float32)
    if isinstance(name, str):   # the reference's own numbers are the reference where there is a fixture (kl's gradients: the difference)
        for k in r64:
            assert np.abs(r64[k][0] - z[k]).max() <= 1e-10 * max(1.0, np.abs(z[k]).max())
            if k == "kl":
                g = {i: z[f"g_cross_entropy_{i}"] - (z[f"g_entropy_{i}"] if i.endswith("_p") else 0.0) for i in INPUTS[k]}
            else:
                g = {i: z[f"g_{k}_{i}"] for i in INPUTS[k]}
            r64[k] = (z[k], g)
    lz_p, _, mud, mua, _, _ = E.dual_batch(*p, ln)
    lz_q = E.dual_batch(*q, ln)[0]
    both = np.maximum(np.abs(lz_p), np.abs(lz_q))
    scales = {"entropy": (lz_p, p, None), "cross_entropy": (both, q, None), "kl": (both, q, p), "risk": (lz_p, c, None)}
    vb = {}
    for k, (lz, v, v_sub) in scales.items():
        vb[k] = []
        for b in range(len(ln)):
            row = lambda t: None if t is None else (t[0][b], t[1][b])
            dd, da = E.direction(p[0][b], p[1][b], int(ln[b]), row(v), row(v_sub))
            weight = float((np.abs(mud[b]) * np.abs(dd)).sum() + (np.abs(mua[b]) * np.abs(da)).sum())
            vb[k].append(max(2e-5 * max(1.0, float(np.abs(lz[b])), weight), 6.0 * abs(float(r32[k][0][b]) - float(r64[k][0][b]))))
    return x, ln, r64, r32, vb


@pytest.mark.parametrize("name", FIXTURES + ("ws",))
@pytest.mark.parametrize("upstream", ("weights", "sum"))
def test_methods_and_gradients(dev, name, upstream):
    from vlgae_amd.torch_struct import DMV1oExpect as DMV1o
    key = WS_N if name == "ws" else name
    x, ln, r64, r32, vb = method_case(key)
    B = len(ln)
    f64 = isinstance(key, str)                      # the fixtures go in as float64 tensors, the restatement case as float32
    dt = torch.float64 if f64 else torch.float32
    wts = np.linspace(-1.5, 2.0, B) if upstream == "weights" else np.ones(B)
    lengths = torch.from_numpy(ln).to(dev)
    worst = {}
    for k in ("entropy", "cross_entropy", "kl", "risk"):
        t = {i: torch.tensor(a, dtype=dt, device=dev, requires_grad=True) for i, a in x.items()}
        dp, dq = DMV1o([t["dec_p"], t["att_p"]], lengths), DMV1o([t["dec_q"], t["att_q"]], lengths)
        val = {"entropy": dp.tree_entropy, "cross_entropy": lambda: dp.tree_cross_entropy(dq), "kl": lambda: dp.tree_kl(dq),
               "risk": lambda: dp.expected_score((t["cost_dec"], t["cost_att"]))}[k]()
        assert val.shape == (B, 1) and val.dtype == dt
        w = torch.tensor(wts, dtype=dt, device=dev).view(B, 1)
        (val.sum() if upstream == "sum" else (val * w).sum()).backward()
        got = val.detach().cpu().numpy().astype(np.float64).reshape(B)
        for b in range(B):
            worst[k] = max(worst.get(k, 0.0), abs(got[b] - r64[k][0][b]) / vb[k][b])
        for i, ten in t.items():
            if i not in INPUTS[k]:
                assert ten.grad is None
                continue
            g = ten.grad.cpu().numpy().astype(np.float64)
            assert ten.grad.dtype == dt and ten.grad.shape == ten.shape and np.isfinite(g).all()
            for b in range(B):
                ref, e32 = r64[k][1][i][b], np.abs(r32[k][1][i][b] - r64[k][1][i][b]).max()
                if (k, i) == ("risk", "cost_dec"):          # the expected counts: STOP probabilities and GO counts, each with its floor
                    worst[f"d{k}/d{i}"] = max(worst.get(f"d{k}/d{i}", 0.0), E.count_ratio(g[b] / wts[b], ref, r32[k][1][i][b]))
                    continue
                bound = (E.mu_bound(e32) if (k, i) == ("risk", "cost_att") else E.grad_bound(ref, e32)) * abs(wts[b])
                err = np.abs(g[b] - wts[b] * ref).max()
                if bound == 0.0:
                    assert err == 0.0, (k, i, b)
                else:
                    worst[f"d{k}/d{i}"] = max(worst.get(f"d{k}/d{i}", 0.0), err / bound)
    report(f"dmv methods {name} upstream={upstream}", worst)


def test_forward_without_gradients_and_partial_costs(dev):
    "no input wants a gradient: the inside-only image; a cost with one member None"
    from vlgae_amd.torch_struct import DMV1oExpect as DMV1o
    dec, attach, v, ln, refs = batch(12, False)
    td, ta, tl = torch.from_numpy(dec).to(dev), torch.from_numpy(attach).to(dev), torch.from_numpy(ln).to(dev)
    d = DMV1o([td, ta], tl)
    r64, r32 = E.dual_batch(dec, attach, ln, (dec, attach)), E.dual_batch(dec, attach, ln, (dec, attach), None, np.float32)
    H = d.tree_entropy()
    assert H.shape == (3, 1) and H.dtype == torch.float32 and not H.requires_grad
    H = H.cpu().numpy().astype(np.float64).reshape(3)
    H64, H32 = r64[0] - r64[1], r32[0].astype(np.float64) - r32[1]
    worst = {}
    for b in range(3):
        dd, da = E.direction(dec[b], attach[b], int(ln[b]), (dec[b], attach[b]))
        weight = np.concatenate([(np.abs(r64[2][b]) * np.abs(dd)).ravel(), (np.abs(r64[3][b]) * np.abs(da)).ravel()])
        worst["H"] = max(worst.get("H", 0.0), abs(H[b] - H64[b]) / E.value_bound(r64[0][b], weight, np.ones_like(weight), abs(H32[b] - H64[b])))
    report("dmv entropy, no gradients", worst)
    # ev is linear in the direction: the dec part and the attach part add up (each of the three within its value bound)
    tv = (torch.from_numpy(v[0]).to(dev), torch.from_numpy(v[1]).to(dev))
    both, only_d, only_a = (d.expected_score(c).cpu().numpy().astype(np.float64).reshape(3) for c in (tv, (tv[0], None), (None, tv[1])))
    for b in range(3):
        dd, da = E.direction(dec[b], attach[b], int(ln[b]), (v[0][b], v[1][b]))
        weight = np.concatenate([(np.abs(refs[0][2][b]) * np.abs(dd)).ravel(), (np.abs(refs[0][3][b]) * np.abs(da)).ravel()])
        assert abs(both[b] - only_d[b] - only_a[b]) <= 3 * E.value_bound(refs[0][0][b], weight, np.ones_like(weight))
    assert not d.expected_score((None, None)).any()


# ---- 3. structural checks (no oracle) -------------------------------------------------------------------------------------------------
STRUCT_NS = (6, 41, WS_N)


@pytest.mark.parametrize("N", STRUCT_NS)
def test_structural_identities(dev, N):
    """Each quantity is held to the bound of the output it is made of, within its sentence: ev to the value bound; sums of mu to the mu
    bound (5e-5, or 6 x the same quantity's error in the float32 restatement); sums and products of hv to the hv bound (1e-4 of the
    largest |hv| in float64, or 6 x the same quantity's error in the float32 restatement).  A length-1 sentence has hv = 0: exact."""
    dec, attach, v, ln, (r64, r32) = batch(N, False)
    worst = {}

    def hold(name, err, bound):
        if bound == 0.0:
            assert err == 0.0, (name, err)
        else:
            worst[name] = max(worst.get(name, 0.0), err / bound)

    f = lambda t: np.asarray(t, np.float64)
    lz, ev, md, ma, hd, ha = (f(t) for t in run_abi(dev, dec, attach, v, None, ln))
    left = np.tril(np.ones((N, N)), -1)[:, :, None]
    go = lambda t_att: np.stack([(t_att * left).sum(1), (t_att * (1 - left)).sum(1)], 1)   # [N, dir, v]: sums over the children on a side
    hv_floor = [1e-4 * max(np.abs(r64[4][b]).max(), np.abs(r64[5][b]).max()) for b in range(3)]
    for b in range(3):
        n = int(ln[b]) + 1
        dd, da = E.direction(dec[b], attach[b], int(ln[b]), (v[0][b], v[1][b]))
        weight = np.concatenate([(np.abs(r64[2][b]) * np.abs(dd)).ravel(), (np.abs(r64[3][b]) * np.abs(da)).ravel()])
        dot32 = float((f(r32[2][b]) * dd).sum() + (f(r32[3][b]) * da).sum())
        hold("ev = <mu, d>", abs(ev[b] - (md[b] * dd).sum() - (ma[b] * da).sum()),
             E.value_bound(r64[0][b], weight, np.ones_like(weight), abs(float(r32[1][b]) - dot32)))
        m32a, m32d, h32a, h32d = f(r32[3][b]), f(r32[2][b]), f(r32[5][b]), f(r32[4][b])
        # every word has one head
        hold("one head", np.abs(ma[b][:, 1:n].sum((0, 2)) - 1).max(), E.mu_bound(np.abs(m32a[:, 1:n].sum((0, 2)) - 1).max()))
        hold("one head, hv", np.abs(ha[b].sum((0, 2))).max(), max(hv_floor[b], 6.0 * np.abs(h32a.sum((0, 2))).max()))
        # every (word, side) stops once
        hold("one stop", np.abs(md[b][1:n, :, :, 1].sum(-1) - 1).max(), E.mu_bound(np.abs(m32d[1:n, :, :, 1].sum(-1) - 1).max()))
        hold("one stop, hv", np.abs(hd[b][:, :, :, 1].sum(-1)).max(), max(hv_floor[b], 6.0 * np.abs(h32d[:, :, :, 1].sum(-1)).max()))
        # GO counts are the sums of the attach counts over that side
        hold("go = row sums", np.abs(md[b][:, :, :, 0] - go(ma[b])).max(), E.mu_bound(np.abs(m32d[:, :, :, 0] - go(m32a)).max()))
        hold("go = row sums, hv", np.abs(hd[b][:, :, :, 0] - go(ha[b])).max(), max(hv_floor[b], 6.0 * np.abs(h32d[:, :, :, 0] - go(h32a)).max()))
        assert not ma[b][:, 0].any() and not ma[b][np.arange(N), np.arange(N)].any() and not ma[b][n:].any() and not ma[b][:, n:].any()
        assert not md[b][n:].any() and not hd[b][n:].any() and not ha[b][n:].any() and not ha[b][:, n:].any()
    # a constant attach direction: every tree has len attachments, <c, tree> is constant and nothing varies
    const = (None, np.full_like(attach, 0.75))
    c32 = E.dual_batch(dec, attach, ln, const, None, np.float32)
    c = run_abi(dev, dec, attach, const, None, ln)
    for b in range(3):
        dd, da = E.direction(dec[b], attach[b], int(ln[b]), (None, const[1][b]))
        weight = (np.abs(r64[3][b]) * np.abs(da)).ravel()
        hold("ev = c len", abs(float(c[1][b]) - 0.75 * ln[b]), E.value_bound(r64[0][b], weight, np.ones_like(weight), abs(float(c32[1][b]) - 0.75 * ln[b])))
        hold("hv = 0", max(np.abs(c[4][b]).max(), np.abs(c[5][b]).max()),
             max(hv_floor[b], 6.0 * max(np.abs(c32[4][b]).max(), np.abs(c32[5][b]).max())))
    # the Hessian is symmetric: <u, Hv> = <v, Hu>
    _, _, u = E.case(N, 900 + N)
    hu = run_abi(dev, dec, attach, u, None, ln)
    u64, u32 = E.dual_batch(dec, attach, ln, u), E.dual_batch(dec, attach, ln, u, None, np.float32)
    for b in range(3):
        du, dv = E.direction(dec[b], attach[b], int(ln[b]), (u[0][b], u[1][b])), E.direction(dec[b], attach[b], int(ln[b]), (v[0][b], v[1][b]))
        dot = lambda d, hd_, ha_: float((d[0] * f(hd_[b])).sum() + (d[1] * f(ha_[b])).sum())
        hold("symmetry", abs(dot(du, hd, ha) - dot(dv, hu[4], hu[5])),
             max(hv_floor[b], 1e-4 * max(np.abs(u64[4][b]).max(), np.abs(u64[5][b]).max()),
                 6.0 * abs(dot(du, r32[4], r32[5]) - dot(dv, u32[4], u32[5]))))
    report(f"dmv structure N={N}", worst)


@pytest.mark.parametrize("N", STRUCT_NS + (255,))
def test_kl_of_a_distribution_with_itself_is_exactly_zero(dev, N):
    from vlgae_amd.torch_struct import DMV1oExpect as DMV1o
    dec, attach = (torch.from_numpy(a).to(dev) for a in batch(N, False)[:2])
    ln = torch.from_numpy(E.ragged(N)).to(dev)
    leaf = lambda: [dec.clone().requires_grad_(True), attach.clone().requires_grad_(True)]
    p, q = leaf(), leaf()
    kl = DMV1o(p, ln).tree_kl(DMV1o(q, ln))
    assert kl.shape == (3, 1)
    (kl * torch.tensor([[1.0], [-2.0], [3.0]], device=dev)).sum().backward()
    assert not kl.detach().any() and all(t.grad is not None and not t.grad.any() for t in p + q)
    assert not DMV1o([dec, attach], ln).tree_kl(DMV1o([dec, attach], ln)).any()          # the inside-only image too
    p = leaf()                                                                          # a fixed q: inside-outside for p, inside only for q
    kl = DMV1o(p, ln).tree_kl(DMV1o([dec, attach], ln))
    kl.sum().backward()
    assert not kl.detach().any() and not p[0].grad.any() and not p[1].grad.any()


@pytest.mark.parametrize("N", STRUCT_NS)
def test_entropy_and_kl_are_nonnegative_and_one_word_has_no_gradient(dev, N):
    from vlgae_amd.torch_struct import DMV1oExpect as DMV1o
    dec, attach, v, ln, refs = batch(N, False)
    dq, aq, _ = E.case(N, 700 + N)
    t = lambda a: torch.from_numpy(a).to(dev)
    p = [t(dec).requires_grad_(True), t(attach).requires_grad_(True)]
    tl = t(ln)
    H = DMV1o(p, tl).tree_entropy()
    H.sum().backward()
    kl = DMV1o([t(dec), t(attach)], tl).tree_kl(DMV1o([t(dq), t(aq)], tl)).cpu().numpy().reshape(3)
    r64 = refs[0]
    for b in range(3):
        w = lambda v_, s_: sum(float((np.abs(m) * np.abs(d)).sum()) for m, d in zip((r64[2][b], r64[3][b]),
                                                                                  E.direction(dec[b], attach[b], int(ln[b]), v_, s_)))
        bound = 2e-5 * max(1.0, abs(r64[0][b]), w((dec[b], attach[b]), None), w((dq[b], aq[b]), (dec[b], attach[b])))
        assert H[b].item() >= -bound and kl[b] >= -bound
        if ln[b] == 1:   # one word, one tree: H = logZ - ev is 0 up to the rounding of two sums of the same potentials; nothing varies, hv = 0 exactly
            assert abs(H[b].item()) <= bound and not p[0].grad[b].any() and not p[1].grad[b].any()


@pytest.mark.parametrize("N", (41, WS_N))   # every chart in LDS | per-sentence workspace slices
def test_a_sentence_does_not_depend_on_its_batch(dev, N):
    dec, attach, v, ln, _ = batch(N, False)
    base = run_abi(dev, dec, attach, v, None, ln)
    od, oa, ov = E.case(N, 9, B=5)
    ov = [ov[0], ov[1]]
    for b in range(3):
        od[4 - b], oa[4 - b], ov[0][4 - b], ov[1][4 - b] = dec[b], attach[b], v[0][b], v[1][b]
    lengths = np.array([min(7, N - 1), N - 1, ln[2], ln[1], ln[0]], np.int64)
    got = run_abi(dev, od, oa, tuple(ov), None, lengths)
    for b in range(3):
        assert all(np.array_equal(x[4 - b], y[b]) for x, y in zip(got, base))


# ---- 4. forbidden entries, bad lengths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (12, WS_N))
def test_forbidden_entries_and_bad_lengths(dev, N):
    rng = np.random.default_rng(40 + N)
    dec, attach, v = E.case(N, 40 + N)
    forbid = rng.random(attach.shape) < 0.2
    forbid[:, np.arange(N - 1), np.arange(1, N)] = False          # the chain 0 -> 1 -> 2 ... stays allowed: the support is not empty
    attach[forbid] = -np.inf
    no_att, no_dec = attach <= -5e11, dec <= -5e11                # the -inf entries and what DMV1o.merge wrote
    v[1][no_att] = 1e30                                           # garbage where nothing may be read
    v[0][no_dec] = 1e30
    ln = E.ragged(N)
    got = run_abi(dev, dec, attach, v, None, ln)
    report(f"dmv forbidden entries N={N}", E.ratios(got, dec, attach, ln, v))
    assert all(np.isfinite(g).all() for g in got)
    assert not got[3][no_att].any() and not got[5][no_att].any() and not got[2][no_dec].any() and not got[4][no_dec].any()
    for bad in (0, N):
        lengths = np.array([ln[0], bad, ln[2]], np.int64)
        out = run_abi(dev, dec, attach, v, None, lengths)
        assert np.isnan(out[0][1]) and np.isnan(out[1][1]) and not any(o[1].any() for o in out[2:])
        for b in (0, 2):                                          # the neighbours: unaffected, bit for bit
            assert all(np.array_equal(x[b], y[b]) for x, y in zip(out, got))
        fw = run_abi(dev, dec, attach, v, None, lengths, grad=False)
        assert np.isnan(fw[0][1]) and np.isnan(fw[1][1]) and np.array_equal(fw[0][[0, 2]], got[0][[0, 2]])


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------------
def test_entropy_with_backward_replays_on_new_potentials(dev):
    """Launches per call, from the code (functional.py): entropy 1 (+ 1 vlg_scale_counts in backward); expected score 1 (+ up to 2);
    cross-entropy and KL 2 (+ 2 in-place subtractions when q wants a gradient, + up to 2 vlg_scale_counts in backward)."""
    from vlgae_amd.torch_struct import DMV1oExpect as DMV1o
    N = 41
    a0, a1 = ([torch.from_numpy(a).to(dev) for a in batch(N, False, seed=s)[:2]] for s in (0, 1))
    ln = torch.from_numpy(E.ragged(N)).to(dev)
    w = torch.tensor([[0.5], [-1.0], [2.0]], device=dev)

    def step(x):
        x[0].grad = x[1].grad = None
        H = DMV1o(x, ln).tree_entropy()
        (H * w).sum().backward()
        return H.detach(), x[0].grad, x[1].grad

    static = [t.clone().requires_grad_(True) for t in a0]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step(static)
    torch.cuda.current_stream(dev).wait_stream(side)
    static[0].grad = static[1].grad = None
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out_g = step(static)
    for new in (a1, a0):
        with torch.no_grad():
            static[0].copy_(new[0])
            static[1].copy_(new[1])
        gr.replay()
        out_e = step([t.clone().requires_grad_(True) for t in new])
        assert all(torch.equal(g, e) for g, e in zip(out_g, out_e))
