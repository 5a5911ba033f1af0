"""CPU: the optimiser step's C ABI (vlg_adam_clip_plan / _workspace / _step) validates on the host before any HIP call, its workspace follows
the chunk plan restated in optim_restatement.py, optim.ClippedAdam resolves its groups by pattern, and the bounds the GPU tests use hold
for float32 torch.optim.Adam itself on the very inputs those tests use."""
import ctypes

import pytest
import torch

import optim_restatement as R


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _table(n=2, **kw):
    from vlgae_amd import _C
    items = (_C.OptTensor * n)()
    for i in range(n):
        items[i] = _C.OptTensor(kw.get("param", 64), kw.get("m", 128), kw.get("v", 256), kw.get("shadow", 32), kw.get("numel", 10), kw.get("lr_mult", 1.0),
                                kw.get("wd", 0.0))
    return items


def test_plan_validates_the_table(lib):
    plan = lib.vlg_adam_clip_plan
    assert plan(_table(), 2) == 0 and plan(_table(shadow=None), 2) == 0        # the shadow is optional
    assert plan(None, 0) == 0 and plan(None, 2) == 0x1003 and plan(_table(), -1) == 0x1001
    assert plan(_table(param=None), 2) == 0x1003 and plan(_table(m=None), 2) == 0x1003 and plan(_table(v=None), 2) == 0x1003
    assert plan(_table(numel=0), 2) == 0x1001 and plan(_table(numel=-3), 2) == 0x1001
    assert plan(_table(lr_mult=-1.0), 2) == 0x1001 and plan(_table(wd=float("nan")), 2) == 0x1001
    for k in ("param", "m", "v"):                                              # float32 arrays: aligned to 4 bytes, and no more than that
        assert plan(_table(**{k: 66}), 2) == 0x1003 and b"4-byte" in lib.vlg_last_error()
        assert plan(_table(**{k: 68}), 2) == 0
    assert plan(_table(shadow=33), 2) == 0x1003 and b"2-byte" in lib.vlg_last_error() and plan(_table(shadow=34), 2) == 0


def test_step_validates_before_any_hip_call(lib):
    from vlgae_amd import _C
    one = ctypes.c_void_p(64)
    numel = (ctypes.c_longlong * 2)(10, 5000)
    need = lib.vlg_adam_clip_workspace(numel, 2)

    def step(**kw):
        hyper = _C.AdamHyper(kw.get("beta1", 0.9), kw.get("beta2", 0.999), kw.get("eps", 1e-12), kw.get("gamma", 1.0), kw.get("max_norm", 5.0))
        grads = (ctypes.c_void_p * 2)(kw.get("g0", 512), 1024)
        dts = (ctypes.c_int * 2)(kw.get("dt0", _C.BF16), _C.F32)
        nm = (ctypes.c_longlong * 2)(kw.get("n0", 10), 5000)
        return lib.vlg_adam_clip_step(kw.get("table", one), nm if kw.get("numel", True) else None, grads if kw.get("grads", True) else None,
                                      dts if kw.get("dts", True) else None, kw.get("count", 2), ctypes.byref(hyper) if kw.get("hyper", True) else None,
                                      kw.get("state", one), kw.get("ws", one), kw.get("ws_bytes", need), None)

    assert step(count=0) == 0 and step(count=0, table=None, state=None, ws=None) == 0                  # nothing to do
    assert step(count=-1) == 0x1001
    for k in ("table", "state", "ws"):
        assert step(**{k: None}) == 0x1003
    for k in ("numel", "grads", "dts", "hyper"):
        assert step(**{k: False}) == 0x1003
    assert step(g0=None) == 0x1003
    assert step(dt0=2) == 0x1002 and step(dt0=-1) == 0x1002
    assert step(n0=0) == 0x1001
    assert step(beta1=1.0) == 0x1001 and step(beta2=-0.1) == 0x1001 and step(eps=-1e-8) == 0x1001 and step(gamma=0.0) == 0x1001
    assert step(max_norm=float("nan")) == 0x1001
    assert step(ws_bytes=need - 1) == 0x1004 and b"workspace" in lib.vlg_last_error()
    assert step(g0=513) == 0x1003 and b"aligned" in lib.vlg_last_error()                              # a bf16 gradient: 2 bytes
    assert step(g0=514, dt0=_C.F32) == 0x1003                                                           # a float32 gradient: 4 bytes
    assert step(state=ctypes.c_void_p(68)) == 0x1003


def test_workspace_follows_the_chunk_plan(lib):
    def query(numels):
        return lib.vlg_adam_clip_workspace((ctypes.c_longlong * len(numels))(*numels), len(numels))

    table = [r["numel"] for r in R.case_table()]
    assert len(table) == R.CAPACITY + 2
    prev = 0
    for count in range(1, len(table) + 1):          # monotone in count, a multiple of 256, and what the restated plan gives
        w = query(table[:count])
        assert w >= prev and w > 0 and w % 256 == 0 and w == R.workspace_bytes(table[:count]), count
        prev = w
    assert query([]) == 0 and query([0]) == 0
    # the squared-sum grid is capped: one slot per workgroup, per launch
    big = [R.CHUNK * (R.NORM_GRID + 7)]
    assert query(big) == R.workspace_bytes(big) == (R.SCALAR_BYTES + 8 * R.NORM_GRID + 255) // 256 * 256
    assert query(big * (R.CAPACITY + 1)) == R.workspace_bytes(big * (R.CAPACITY + 1)) == (R.SCALAR_BYTES + 8 * 2 * R.NORM_GRID + 255) // 256 * 256


def test_chunk_plan_of_the_case_table():
    """Which (launch, tensor, offset, length) every chunk covers, pinned; every element is covered exactly once."""
    from vlgae_amd import optim
    assert (optim.CHUNK, optim.CAPACITY) == (R.CHUNK, R.CAPACITY) == (4096, 128)
    numels = [r["numel"] for r in R.case_table()]
    plan = R.chunk_plan(numels)
    C = R.CHUNK
    assert plan[:6] == [(0, i, 0, n) for i, n in enumerate((1, 2, 3, 7, 8, 9))]
    assert plan[6:13] == [(0, 6, 0, C - 1), (0, 7, 0, C), (0, 8, 0, C), (0, 8, C, 1), (0, 9, 0, C), (0, 9, C, C), (0, 9, 2 * C, 5)]
    assert [c for c in plan if c[0] == 1] == [(1, 128, 0, numels[128]), (1, 129, 0, numels[129])]
    assert R.launches(numels) == [(131, 131, 131), (2, 2, 2)]
    cover = [torch.zeros(n, dtype=torch.int32) for n in numels]
    for launch, i, lo, length in plan:
        assert launch == i // R.CAPACITY and 0 < length <= C and lo % C == 0
        cover[i][lo:lo + length] += 1
    assert all(bool((c == 1).all()) for c in cover)


class _FakeStep:
    def __init__(self, P, names):
        self.P, self.names = P, names


def test_for_step_resolves_groups_by_pattern(lib):
    from vlgae_amd import optim
    P = {k: torch.zeros(4, dtype=torch.bfloat16 if k.startswith("ff.") else torch.float32) for k in
         ("emb", "ff.head_ff.linear.weight", "ff.mid_ff.linear1.bias", "ln_w", "w_ff.x", "w1")}
    step = _FakeStep(P, sorted(P))
    opt = optim.ClippedAdam.for_step(step, lr=1e-3, weight_decay=0.1, groups=[{"pattern": r"ff\.mid", "lr_mult": 0.25},
                                                                              {"pattern": r"ff\.", "lr_mult": 2.0, "weight_decay": 0.0},
                                                                              {"pattern": r"ln_", "weight_decay": 0.0}])
    assert opt.names == ["ff.head_ff.linear.weight", "ff.mid_ff.linear1.bias", "ln_w", "w1", "w_ff.x"]     # the frozen features are data
    assert opt.options == {"ff.head_ff.linear.weight": (2.0, 0.0), "ff.mid_ff.linear1.bias": (0.25, 0.1),   # first match; re.match anchors at the start
                           "ln_w": (1.0, 0.0), "w1": (1.0, 0.1), "w_ff.x": (1.0, 0.1)}
    # a bf16 leaf is the shadow of a float32 master initialised from it; a float32 leaf is its own master
    assert opt.master["ln_w"].data_ptr() == P["ln_w"].data_ptr() and opt.shadow["ln_w"] is None
    assert opt.master["ff.head_ff.linear.weight"].dtype == torch.float32 and opt.shadow["ff.head_ff.linear.weight"].data_ptr() == P["ff.head_ff.linear.weight"].data_ptr()
    assert int(opt.count) == 0 and float(opt.lr) == pytest.approx(1e-3) and all(float(v.abs().sum()) == 0 for v in opt.exp_avg.values())
    sd = opt.state_dict()
    assert sorted(sd) == ["exp_avg", "exp_avg_sq", "master", "state"] and sd["master"]["w1"].data_ptr() != opt.master["w1"].data_ptr()
    opt.load_state_dict(sd)
    with pytest.raises(ValueError):
        optim.ClippedAdam({"w": torch.zeros(4, 4).t()})                    # not contiguous: it would have to be copied
    with pytest.raises(ValueError):
        optim.ClippedAdam({"w": torch.zeros(4, dtype=torch.float64)})
    with pytest.raises(ValueError):
        optim.ClippedAdam({"w": torch.zeros(4)}, groups=[{"pattern": "w", "lr": 1.0}])
    with pytest.raises(ValueError):
        opt.update({k: torch.zeros(4) for k in opt.names if k != "w1"})     # a missing gradient
    with pytest.raises(RuntimeError, match="MI355X"):
        opt.update({k: torch.zeros(4) for k in opt.names})                  # host tensors never reach the launch


def _torch32(p0, grads, opts, **kw):
    """float32 torch on the CPU: p, m, v and its own norm.  coef and lr are not torch's results (the oracle forms them in Python from the
    norm): the 2^-22 bounds on them are for the kernel, whose norm is accumulated in float64."""
    got = R.oracle(p0, grads, opts, torch.float32, **kw)
    return {k: v for k, v in got.items() if k not in ("coef", "lr")}


def _scale(regime, p0, grads, opts):
    return R.absolute_scale(p0, grads, opts) if regime == "mixed" else None


@pytest.mark.parametrize("regime", R.REGIMES)
def test_float32_torch_meets_the_bounds(regime):
    """The bounds are validated by torch alone: float32 torch.optim.Adam on the CPU, on the inputs of the GPU case table, stays inside them
    against the float64 run."""
    ref = R.oracle64(regime)
    _, p0, grads = R.draw(regime)
    opts = list(R.options(R.case_table()).values())
    R.check_against(ref, _torch32(p0, grads, opts), opts, R.K, what=regime, scale=_scale(regime, p0, grads, opts))
    if regime in ("zero", "five"):
        assert ref["norm"] == {"zero": [0.0] * 3, "five": [5.0] * 3}[regime]
    else:
        assert all(30 < n < 50 for n in ref["norm"]), ref["norm"]
    if regime == "five":
        assert all(0.999999 < c < 1.0 for c in ref["coef"])
    if regime == "mixed":      # the signs do change: m cancels and g + weight_decay p has opposite signs somewhere
        assert any(bool(((grads[0][i] * grads[1][i]) < 0).any()) for i in range(len(p0)))
        assert any(wd > 0 and bool(((grads[0][i].float() * p0[i].float()) < 0).any()) for i, (_, wd) in enumerate(opts))


def test_float32_torch_meets_the_bounds_without_clipping_and_with_an_lr_change():
    _, p0, grads = R.draw("forty")
    opts = list(R.options(R.case_table()).values())
    for kw in (dict(max_norm=None), dict(lr_scale_before={1: 0.5})):
        ref = R.oracle(p0, grads, opts, torch.float64, **kw)
        R.check_against(ref, _torch32(p0, grads, opts, **kw), opts, R.K, what=str(kw))


@pytest.mark.parametrize("regime", ("forty", "mixed"))
def test_float32_torch_meets_the_bounds_over_the_captured_sequence(regime):
    """The five updates of the captured-update GPU test (two warm-up updates, three replays), at K = 5."""
    _, p0, grads = R.draw(regime)
    opts = list(R.options(R.case_table()).values())
    seq = [grads[k] for k in R.CAPTURED_ORDER]
    ref = R.oracle(p0, seq, opts, torch.float64)
    R.check_against(ref, _torch32(p0, seq, opts), opts, len(seq), what=regime + " x5", scale=_scale(regime, p0, grads, opts))


def test_max_norm_must_be_positive():
    from vlgae_amd import optim
    for bad in (0.0, -1.0):      # torch's clip_grad_norm_(..., 0) zeroes the gradients; "no clipping" is None / inf
        with pytest.raises(ValueError, match="max_norm"):
            optim.ClippedAdam({"w": torch.zeros(4)}, max_norm=bad)
    optim.ClippedAdam({"w": torch.zeros(4)}, max_norm=float("inf"))
