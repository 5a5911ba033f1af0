"""The optimiser step between two training steps, on the device: global-norm clipping, Adam, the exponential learning-rate decay and the
refresh of the bf16 tensors the step reads, as two launches (csrc/vlg_optim.hip; include/vlgae_amd.h `vlg_adam_clip_*`).

What the reference runs after `loss.backward()` (src/pipeline.py:176-227, config/trainer/train.yaml:14, config/model/optimize/linear.yaml):
`clip_grad_norm_(params, 5.)`, `torch.optim.Adam(lr=1e-3, betas=(0.9, 0.999), eps=1e-12).step()`, `ExponentialLR(gamma=0.75 ** (1 / 2000)).step()`.

    opt = optim.ClippedAdam.for_step(step, lr=1e-3, eps=1e-12, gamma=0.75 ** (1 / 2000), max_norm=5.0)
    loss, grads, _ = step()
    opt.update(grads)            # step.P is updated in place: the next step() reads the new values

Every bf16 tensor gets a float32 master (initialised from it) and becomes the master's SHADOW: the update pass writes bf16(master) into
the very tensor the step holds.  A float32 tensor is its own master.  The update count, the base learning rate and the last update's norm /
clip coefficient / learning rate live in device memory (`opt.count`, `opt.lr`, `opt.last_norm`, `opt.last_coef`, `opt.last_lr`: views, read
them when convenient); `update` makes no host synchronisation and no copy, and can be captured in a HIP graph (the kernels advance the
count: every replay is a new step).  `opt.lr.fill_(x)` between updates serves a host-driven scheduler (the reference's ReduceLROnPlateau).
"""
import ctypes
import math
import re

import torch

from . import _C

CHUNK = 4096        # elements per chunk (kOptChunk of csrc/vlg_optim.hip)
CAPACITY = 128      # tensors per launch (kOptCapacity)
FROZEN = ("emb", "vis_box_feat")   # leaves of a step that are data (frozen features), not parameters: train_step's `step.trainable` excludes them
_DT = {torch.float32: _C.F32, torch.bfloat16: _C.BF16}


def resolve_groups(names, groups, lr_mult=1.0, weight_decay=0.0):
    """{name: (lr_mult, weight_decay)}: the first group whose `pattern` re.match-es the name decides (as src/pipeline.py:186-201 picks a
    parameter's options); a group gives "lr_mult" and / or "weight_decay", what it leaves out and every unmatched name take the defaults."""
    compiled = [(re.compile(g["pattern"]), g) for g in (groups or ())]
    for _, g in compiled:
        unknown = set(g) - {"pattern", "lr_mult", "weight_decay"}
        if unknown:
            raise ValueError(f"optim: unknown group options {sorted(unknown)} (pattern, lr_mult, weight_decay)")
    out = {}
    for name in names:
        opts = next((g for rx, g in compiled if rx.match(name)), {})
        out[name] = (float(opts.get("lr_mult", lr_mult)), float(opts.get("weight_decay", weight_decay)))
    return out


class ClippedAdam:
    """clip_grad_norm_ + Adam + ExponentialLR + bf16 refresh over `params` {name: tensor}, updated IN PLACE.

    params: float32 or bfloat16 tensors on one device, contiguous (a tensor that would have to be copied is refused with a ValueError: the
    copy, not the caller's tensor, would be updated).  max_norm None / inf: no clipping (the norm is still reported).  groups: see
    `resolve_groups`.  gamma: the learning rate of update k is lr * lr_mult * gamma ** (k - 1).  storage: an advanced hook, used by
    the tests to place every array at an odd offset -- {"master" | "exp_avg" | "exp_avg_sq": {name: float32 tensor}}, the caller's memory
    for those tensors instead of new allocations; element alignment is all it needs.  Entries must not overlap each other or a parameter:
    that is the caller's to ensure, it is not checked."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-12, weight_decay=0.0, gamma=1.0, max_norm=None, groups=None, storage=None):
        self.names = list(params)
        if not self.names:
            raise ValueError("optim.ClippedAdam: no parameters")
        tensors = [params[k] for k in self.names]
        dev = tensors[0].device
        for k, t in zip(self.names, tensors):
            if t.device != dev or not t.is_contiguous() or t.dtype not in _DT or t.numel() == 0:
                raise ValueError(f"optim.ClippedAdam: parameter {k!r} ({t.dtype}, {t.device}, contiguous={t.is_contiguous()}, numel={t.numel()}) would have to be "
                                 f"copied -- pass float32 / bfloat16 tensors on one device ({dev}), contiguous and not empty")
        max_norm = math.inf if max_norm is None else float(max_norm)
        if max_norm <= 0.0:   # (torch's clip_grad_norm_(..., 0) zeroes the gradients; the C entry reads <= 0 as "no clipping": refuse it here)
            raise ValueError(f"optim.ClippedAdam: max_norm={max_norm} (positive, or None / inf for no clipping)")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0 and gamma > 0.0 and lr >= 0.0) or math.isnan(max_norm):
            raise ValueError(f"optim.ClippedAdam: lr={lr} betas={betas} eps={eps} gamma={gamma} max_norm={max_norm}")
        self.device = dev
        self.options = resolve_groups(self.names, groups, 1.0, weight_decay)
        self.params = dict(zip(self.names, tensors))
        storage = storage or {}

        def own(kind, k, like):
            """float32 memory for `kind` of parameter k: the caller's `storage[kind][k]` or a new tensor."""
            t = storage.get(kind, {}).get(k)
            if t is None:
                return torch.empty(like.shape, dtype=torch.float32, device=dev)
            if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() != like.numel():
                raise ValueError(f"optim.ClippedAdam: storage[{kind!r}][{k!r}] must be float32 on {dev}, contiguous, with {like.numel()} elements")
            return t.detach()

        with torch.no_grad():
            # a bf16 tensor is the shadow of a float32 master initialised from it; a float32 tensor is its own master
            self.master = {}
            self.shadow = {k: (t.detach() if t.dtype == torch.bfloat16 else None) for k, t in self.params.items()}
            for k, t in self.params.items():
                if t.dtype == torch.bfloat16:
                    self.master[k] = own("master", k, t)
                    self.master[k].view(-1).copy_(t.detach().view(-1))
                else:
                    self.master[k] = t.detach()
            self.exp_avg = {k: own("exp_avg", k, t).zero_() for k, t in self.master.items()}
            self.exp_avg_sq = {k: own("exp_avg_sq", k, t).zero_() for k, t in self.master.items()}
            # int64 count | float32 lr, last norm, last coef, last lr | padding: 32 bytes the kernels read and write
            self.state = torch.zeros(8, dtype=torch.float32, device=dev)
            self.state[2] = lr
        self.count = self.state[:2].view(torch.int64)[0]
        self.lr, self.last_norm, self.last_coef, self.last_lr = self.state[2], self.state[3], self.state[4], self.state[5]
        self.hyper = _C.AdamHyper(betas[0], betas[1], eps, gamma, max_norm)
        n = len(self.names)
        items = (_C.OptTensor * n)()
        for i, k in enumerate(self.names):
            sh = self.shadow[k]
            items[i] = _C.OptTensor(self.master[k].data_ptr(), self.exp_avg[k].data_ptr(), self.exp_avg_sq[k].data_ptr(), None if sh is None else sh.data_ptr(),
                                    self.master[k].numel(), *self.options[k])
        lib = _C.lib()
        _C.check(lib.vlg_adam_clip_plan(items, n), "adam_clip_plan")
        # the table on the device, written once (the one synchronous copy)
        self.table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
        self._numel = (ctypes.c_longlong * n)(*[self.master[k].numel() for k in self.names])
        self._grads, self._dtypes = (ctypes.c_void_p * n)(), (ctypes.c_int * n)()
        self.ws_bytes = lib.vlg_adam_clip_workspace(self._numel, n)
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=dev)

    @classmethod
    def for_step(cls, step, names=None, **kw):
        """Over the trainable leaves of a built training step: `step.names` without the frozen features (`emb`, `vis_box_feat`: data), or
        `names`.  The leaves `step.P[name]` are updated in place (a bf16 leaf as the shadow of its float32 master)."""
        if names is None:
            names = [k for k in step.names if k not in FROZEN]
        return cls({k: step.P[k] for k in names}, **kw)

    def update(self, grads):
        """One update from `grads` {name: gradient} (what step() returns, or views into a gradient bucket): float32 or bfloat16, on the
        optimiser's device, of the parameter's element count.  A non-contiguous gradient is copied into a contiguous one first (one more
        launch and pass over it); entries for other names are ignored.  The gradients are not changed."""
        copies = []   # contiguous copies stay referenced until the launches are enqueued: the allocator would hand a freed one to the next copy
        for i, k in enumerate(self.names):
            if k not in grads:
                raise ValueError(f"optim.ClippedAdam.update: no gradient for {k!r}")
            g = grads[k]
            if g.dtype not in _DT or g.device != self.device or g.numel() != self._numel[i]:
                raise ValueError(f"optim.ClippedAdam.update: gradient of {k!r}: {g.dtype} on {g.device} with {g.numel()} elements (float32 / bfloat16 "
                                 f"on {self.device} with {self._numel[i]})")
            if not g.is_contiguous():
                g = g.contiguous()
                copies.append(g)
            self._grads[i], self._dtypes[i] = g.data_ptr(), _DT[g.dtype]
        _C.require_gpu(self.state, "optim.ClippedAdam.update")
        _C.check(_C.lib().vlg_adam_clip_step(_C.ptr(self.table), self._numel, self._grads, self._dtypes, len(self.names), ctypes.byref(self.hyper),
                                             _C.ptr(self.state), _C.ptr(self.ws), self.ws_bytes, _C.stream_of(self.state)), "adam_clip_step")

    def state_dict(self):
        """Copies of the masters, exp_avg, exp_avg_sq (by name) and of the device state (count, lr, last norm / coef / lr): torch.save-able."""
        clone = lambda d: {k: t.detach().clone() for k, t in d.items()}
        return dict(master=clone(self.master), exp_avg=clone(self.exp_avg), exp_avg_sq=clone(self.exp_avg_sq), state=self.state.detach().clone())

    def load_state_dict(self, sd):
        """Copy a state_dict into this optimiser's own tensors (addresses stay) and rewrite every shadow from its master."""
        if set(sd["master"]) != set(self.names):
            raise ValueError(f"optim.ClippedAdam.load_state_dict: names differ: {sorted(set(sd['master']) ^ set(self.names))}")
        with torch.no_grad():
            for mine, theirs in ((self.master, sd["master"]), (self.exp_avg, sd["exp_avg"]), (self.exp_avg_sq, sd["exp_avg_sq"])):
                for k in self.names:
                    mine[k].view(-1).copy_(theirs[k].reshape(-1))
            self.state.copy_(sd["state"])
            for k, sh in self.shadow.items():
                if sh is not None:
                    sh.view(-1).copy_(self.master[k].view(-1))
