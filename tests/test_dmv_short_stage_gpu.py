"""GPU: the short image's load stage and count write-out after round 13 -- the potentials requested at kernel entry for all N rows of the
tensor, ahead of lengths[b]; every chart cell stored once by one lane; the counts read from LDS with every read of a lane in flight
together -- against the general image, bit for bit.

The embedding method of test_dmv_short_hold_gpu.py: a batch at tensor width N <= 41 launches the short image; the same batch embedded
into N = 42 tensors filled with the semiring zero launches the general image, which this round does not touch.  Outputs are compared
through int32 views (the bits, not the values: -0 is not +0 and a NaN is its pattern).

  * widths N = 2, 3, 5, 6, 41 with every length 1 ... N - 1 in one batch: the GO row sums meet n = 0, 1, 4, 5, 40 cells and a lane
    owns one to four attach cells;
  * entries: merged fused Log with a unit and a non-unit cotangent, Log inside only, Max with the back-pointer walk, decode with
    `heads` (the write-out keeps its barrier there), the marginals + Viterbi pair launch, the rule-table entry;
  * float32 and bf16 storage; random, tied and -inf potentials;
  * every launch runs twice, and every launch that takes its outputs from the caller a third time into outputs pre-filled with NaN
    (int64: -1): identical bits, and exact zeros at every padded position (the rule-table launcher allocates and zero-fills its own);
  * poisoned padding: at N = 41 with lengths 1, 2, 17, 39 the positions >= Ne of dec and attach and attach's diagonal hold NaN, +inf,
    -inf and 3e38 (the stage now READS them and must discard them by select): the outputs equal those with zeros there;
  * invalid lengths 0 and N beside valid neighbours: NaN logZ and zero counts for them (their requests lapse), the neighbours unchanged."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu

SR_LOG, SR_MAX = 0, 1
WIDE = 42   # one past kShortN: the general image
WIDTHS = [2, 3, 5, 6, 41]
DTYPES = [torch.float32, torch.bfloat16]
KINDS = ["random", "tied", "neginf"]


@pytest.fixture(scope="module")
def Fn():
    import vlgae_amd.torch_struct.functional as F
    return F


@pytest.fixture(scope="module")
def oracle_mod():
    import oracle
    oracle.build()
    return oracle


def make_batch(oracle_mod, N, kind, lengths, seed):
    """merged potentials and rule tables of the sentences `lengths` at tensor width N"""
    rng = np.random.default_rng(seed)
    L = N - 1
    lengths = np.asarray(lengths, dtype=np.int64)
    B = len(lengths)
    T = L + 1
    if kind == "tied":   # a handful of values, all exact in bf16: most maxima and many sums are ties
        dec = np.log(rng.choice([0.25, 0.5, 0.75], (B, L, 2, 2, 2))).astype(np.float32)
        attach = rng.choice([-1.0, -0.5, 0.0], (B, L, L, 2)).astype(np.float32)
        root = np.full((B, L), np.log(0.5), np.float32)
        rule = rng.choice([-1.0, -0.5, 0.0], (B, L, T, 2, 2)).astype(np.float32)
        rroot = np.full(T, np.log(0.5), np.float32)
    else:
        dec = np.log(rng.dirichlet(np.ones(2), (B, L, 2, 2))).astype(np.float32)
        attach = rng.standard_normal((B, L, L, 2)).astype(np.float32)
        root = np.log(rng.dirichlet(np.ones(L), B)).astype(np.float32)
        rule = rng.standard_normal((B, L, T, 2, 2)).astype(np.float32)
        rroot = np.log(rng.dirichlet(np.ones(T))).astype(np.float32)
    md, ma = oracle_mod.dmv1o_merge(dec, attach, root)
    token = np.stack([rng.permutation(T)[:L] for _ in range(B)]).astype(np.int64)   # a token of its own per word: one atomic add per rule word
    if kind == "neginf":   # the chain 0 -> 1 -> 2 -> ... is left alone, so every sentence keeps a finite tree
        forbid = rng.random(ma.shape[:3]) < 0.1
        forbid[:, np.arange(N - 1), np.arange(1, N)] = False
        ma = ma.copy()
        ma[forbid] = -np.inf
        b, h, c = np.nonzero(forbid[:, 1:, 1:])
        keep = h != c
        b, h, c = b[keep], h[keep], c[keep]
        rule[b, h, token[b, c], np.where(c < h, 0, 1)] = -np.inf
    g = (0.25 + 2.5 * rng.random(B)).astype(np.float32)
    return dict(md=md, ma=ma, lengths=lengths, g=g, dec=dec, rule=rule, rroot=rroot, token=token)


@pytest.fixture(scope="module")
def batches(oracle_mod):
    """(N, kind) -> every length 1 ... N - 1 in one batch, made once and shared by both storage types"""
    made = {}

    def get(N, kind):
        if (N, kind) not in made:
            made[(N, kind)] = make_batch(oracle_mod, N, kind, np.arange(1, N), 1300 + 10 * N + KINDS.index(kind))
        return made[(N, kind)]

    return get


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def embedded(a, fill, square, width=WIDE):
    """a [B,n,...] (square: [B,n,n,...]) placed in the leading corner of a `width`-wide tensor filled with `fill`"""
    B, n = a.shape[:2]
    out = np.full((B, width, width) + a.shape[3:] if square else (B, width) + a.shape[2:], fill, a.dtype)
    if square:
        out[:, :n, :n] = a
    else:
        out[:, :n] = a
    return out


def fresh(shape, dtype, dev, stale):
    """an output buffer: uninitialised, or holding what no launch may leave behind"""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    if not stale:
        return torch.empty(shape, dtype=dtype, device=dev)
    return torch.full(shape, -1 if dtype == torch.int64 else float("nan"), dtype=dtype, device=dev)


def pair_launch(d, a, ln, stale):
    """vlg_dmv1o_marginals_viterbi with every output kept: (logZ, grad_dec, grad_attach, best, tree dec counts, tree attach counts, heads)"""
    from vlgae_amd import _C
    B, N = d.shape[:2]
    assert _C.lib().vlg_dmv1o_marginals_viterbi_supported(N)
    dt, dc = _C.in_dtype(d)
    _, ac = _C.in_dtype(a)
    dev = d.device
    f32 = torch.float32
    logZ, best = fresh(B, f32, dev, stale), fresh(B, f32, dev, stale)
    gdec, vdec = (fresh((B, N, 2, 2, 2), f32, dev, stale) for _ in range(2))
    gatt, vatt = (fresh((B, N, N, 2), f32, dev, stale) for _ in range(2))
    heads = fresh((B, N), torch.int64, dev, stale)
    _C.check(_C.lib().vlg_dmv1o_marginals_viterbi(_C.ptr(dc), _C.ptr(ac), _C.ptr(ln), B, N, dt, _C.ptr(logZ), _C.ptr(gdec), _C.ptr(gatt),
                                                  _C.ptr(best), _C.ptr(vdec), _C.ptr(vatt), _C.ptr(heads), _C.stream_of(d)),
             "dmv1o_marginals_viterbi")
    return logZ, gdec, gatt, best, vdec, vatt, heads


MERGED = ("fused_unit", "fused_g", "inside", "max_walk", "decode", "pair")


def merged_launches(Fn, md, ma, lengths, g, dtype, stale=False):
    """every entry that takes merged potentials, each with all of its outputs"""
    d, a, ln, gl = t(md).to(dtype), t(ma).to(dtype), t(lengths), t(g)
    B, N = d.shape[:2]
    dev, f32 = d.device, torch.float32

    def outs3():
        return fresh(B, f32, dev, stale), fresh((B, N, 2, 2, 2), f32, dev, stale), fresh((B, N, N, 2), f32, dev, stale)

    return {
        "fused_unit": Fn.dmv1o_run(d, a, ln, SR_LOG, True, out=outs3()),
        "fused_g": Fn.dmv1o_run(d, a, ln, SR_LOG, True, grad_logZ=gl, out=outs3()),
        "inside": Fn.dmv1o_run(d, a, ln, SR_LOG, False, out=(fresh(B, f32, dev, stale), None, None))[:1],
        "max_walk": Fn.dmv1o_run(d, a, ln, SR_MAX, True, out=outs3()),
        "decode": Fn.dmv1o_decode(d, a, ln, out=(fresh(B, f32, dev, stale), fresh((B, N), torch.int64, dev, stale))),
        "pair": pair_launch(d, a, ln, stale),
    }


def rules_launch(Fn, x, dtype, wide, zero):
    dec, rule, token = x["dec"], x["rule"], x["token"]
    if wide:
        dec, rule = embedded(dec, zero, False, WIDE - 1), embedded(rule, zero, False, WIDE - 1)
        token = embedded(token, 0, False, WIDE - 1)
    args = (t(rule).to(dtype), t(dec).to(dtype), t(x["rroot"]).to(dtype), t(token), t(x["lengths"]))
    r = Fn.dmv1o_rules_run(*args, SR_LOG, True, grad_logZ=t(x["g"]))
    v = Fn.dmv1o_rules_run(*args, SR_MAX, False, want_heads=True)   # the rule-table decode: the head vector of the best tree
    return r["logZ"], r["grad_dec"], r["grad_rule"], r["grad_root"], v["logZ"], v["heads"]


# how an output of the wide launch is cut back to the short one's shape: None: as it is, "row": [:, :n], "square": [:, :n, :n]
CUTS = {
    "fused_unit": (None, "row", "square"),
    "fused_g": (None, "row", "square"),
    "inside": (None,),
    "max_walk": (None, "row", "square"),
    "decode": (None, "row"),
    "pair": (None, "row", "square", None, "row", "square", "row"),
    "rules": (None, "row", "row", None, None, "row"),
}


def cut(w, how, n):
    if how is None:
        return w
    return w[:, :n, :n] if how == "square" else w[:, :n]


def bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def assert_padding_is_zero(what, outs, cuts, lengths):
    """every output with a position axis: exact zeros at the positions past the sentence (rows, and columns of a square)"""
    ln = t(lengths)
    for k, (o, how) in enumerate(zip(outs, cuts)):
        if how is None:
            continue
        pad = torch.arange(o.shape[1], device=o.device)[None, :] > ln[:, None]   # position p of the root-augmented sentence: padding when p > len
        if how == "square":
            m = (pad[:, :, None] | pad[:, None, :])
            assert bool((bits(o)[m] == 0).all()), f"{what}: output {k} is not exactly zero at a padded cell"
        else:
            assert bool((bits(o)[pad] == 0).all()), f"{what}: output {k} is not exactly zero at a padded position"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_entry_equals_the_general_image(Fn, oracle_mod, batches, kind, dtype):
    zero = np.float32(oracle_mod.NEGINF)
    for N in WIDTHS:
        x = batches(N, kind)
        what = f"N={N} {kind}"
        short = merged_launches(Fn, x["md"], x["ma"], x["lengths"], x["g"], dtype)
        again = merged_launches(Fn, x["md"], x["ma"], x["lengths"], x["g"], dtype)
        stale = merged_launches(Fn, x["md"], x["ma"], x["lengths"], x["g"], dtype, stale=True)
        wide = merged_launches(Fn, embedded(x["md"], zero, False), embedded(x["ma"], zero, True), x["lengths"], x["g"], dtype)
        short["rules"], again["rules"], wide["rules"] = (rules_launch(Fn, x, dtype, w, zero) for w in (False, False, True))
        torch.cuda.synchronize()
        for launch, cuts in CUTS.items():
            assert len(short[launch]) == len(cuts)
            assert bool(torch.isfinite(short[launch][0]).all()), f"{what} {launch}: the score is not finite"
            # (the rule-table launcher allocates and zero-fills its outputs itself: no run into pre-filled buffers for it)
            for k, (s, s2, s3, w, how) in enumerate(zip(short[launch], again[launch], stale.get(launch, short[launch]), wide[launch], cuts)):
                c = cut(w, how, s.shape[1] if s.dim() > 1 else 0)
                assert same_bits(s, s2), f"{what} {launch}: output {k} differs between two calls"
                assert launch not in stale or same_bits(s, s3), f"{what} {launch}: output {k} depends on what its buffer held before"
                assert same_bits(s, c), f"{what} {launch}: output {k} differs between the short and the general image"
            if launch != "rules":   # rule space: positions are words, checked against the general image above
                assert_padding_is_zero(f"{what} {launch}", stale[launch], cuts, x["lengths"])
        # the launches agree with each other where they compute the same thing
        for k in range(3):
            assert same_bits(short["pair"][k], short["fused_unit"][k])
        assert same_bits(short["inside"][0], short["fused_unit"][0])
        assert float(short["fused_unit"][2].abs().sum()) > 0 and float(short["rules"][2].abs().sum()) + float(short["rules"][3].abs().sum()) > 0
        # the best tree has one head per word
        assert torch.equal(short["max_walk"][2].sum((1, 2, 3)), t(x["lengths"]).to(torch.float32)), f"{what}: the best tree is not a tree"


POISON_F32 = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(3e38)]
POISON_BF16 = [0x7FC0, 0xFFFF, 0x7F80, 0xFF80, 0x7F61]   # quiet NaNs of both signs, +inf, -inf, 3e38 -- as bf16 patterns


def poisoned(md, ma, lengths, dtype, rng):
    """device tensors of storage `dtype` with every position >= Ne of dec and attach, and attach's whole diagonal, overwritten"""
    B, N = md.shape[:2]
    pos = np.arange(N)
    pad = pos[None, :] > np.asarray(lengths)[:, None]
    mask_d = np.broadcast_to(pad[:, :, None, None, None], md.shape)
    mask_a = np.broadcast_to((pad[:, :, None] | pad[:, None, :] | np.eye(N, dtype=bool)[None])[..., None], ma.shape)
    d, a = t(md).to(dtype), t(ma).to(dtype)
    for x, mask in ((d, mask_d), (a, mask_a)):
        m = t(np.ascontiguousarray(mask))
        if dtype == torch.float32:
            x[m] = t(rng.choice(POISON_F32, int(mask.sum())))
        else:
            x.view(torch.int16)[m] = t(rng.choice(POISON_BF16, int(mask.sum())).astype(np.uint16).view(np.int16))
    return d, a


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_poisoned_padding_and_diagonal_change_nothing(Fn, oracle_mod, dtype):
    N, lengths = 41, [1, 2, 17, 39]
    x = make_batch(oracle_mod, N, "random", lengths, 1391)
    rng = np.random.default_rng(1392)
    pad = np.arange(N)[None, :] > np.asarray(lengths)[:, None]
    md, ma = x["md"].copy(), x["ma"].copy()
    md[pad] = 0
    ma[pad[:, :, None] | pad[:, None, :] | np.eye(N, dtype=bool)[None]] = 0
    clean = merged_launches(Fn, md, ma, x["lengths"], x["g"], dtype)
    d, a = poisoned(md, ma, lengths, dtype, rng)
    assert not bool(torch.isfinite(a.float()).all()) and not bool(torch.isfinite(d.float()).all())
    ln, gl = t(x["lengths"]), t(x["g"])
    dirty = {
        "fused_unit": Fn.dmv1o_run(d, a, ln, SR_LOG, True),
        "fused_g": Fn.dmv1o_run(d, a, ln, SR_LOG, True, grad_logZ=gl),
        "inside": Fn.dmv1o_run(d, a, ln, SR_LOG, False)[:1],
        "max_walk": Fn.dmv1o_run(d, a, ln, SR_MAX, True),
        "decode": Fn.dmv1o_decode(d, a, ln),
        "pair": pair_launch(d, a, ln, False),
    }
    torch.cuda.synchronize()
    for launch in MERGED:
        assert bool(torch.isfinite(clean[launch][0]).all())
        for k, (c, p) in enumerate(zip(clean[launch], dirty[launch])):
            assert same_bits(c, p), f"{launch}: output {k} changes with what the padding and the diagonal hold"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_invalid_lengths_beside_valid_neighbours(Fn, oracle_mod, dtype):
    for N in (3, 6, 41):
        valid = [min(N - 1, k) for k in (1, 2, N - 1, N // 2 + 1, N - 1, 1)]
        x = make_batch(oracle_mod, N, "random", valid, 1393 + N)
        bad = np.array(valid)
        bad[[1, 4]] = (0, N)   # not sentences: each between two that are
        good = merged_launches(Fn, x["md"], x["ma"], x["lengths"], x["g"], dtype)
        mixed = merged_launches(Fn, x["md"], x["ma"], bad, x["g"], dtype, stale=True)
        torch.cuda.synchronize()
        inv, ok = t(np.isin(np.arange(len(valid)), [1, 4])), t(~np.isin(np.arange(len(valid)), [1, 4]))
        for launch in MERGED:
            for k, (gd, mx) in enumerate(zip(good[launch], mixed[launch])):
                what = f"N={N} {launch}: output {k}"
                assert same_bits(gd[ok], mx[ok]), f"{what} of a valid sentence changes beside an invalid one"
                if gd.dim() == 1:
                    assert bool(torch.isnan(mx[inv]).all()), f"{what}: the score of an invalid sentence is not NaN"
                else:
                    assert bool((bits(mx[inv]) == 0).all()), f"{what}: an invalid sentence has a non-zero count"
