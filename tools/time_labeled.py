"""DependencyCRF on labeled potentials [B,N,N,L] beside its two yardsticks, each as a replayed HIP graph.
    python tools/time_labeled.py [--out=FILE] [--replays=N] [--repeats=R]
    python tools/time_labeled.py --resources [--out=FILE]     # no GPU: (re)write only the kernels' register / LDS figures into FILE

Per shape -- B = 256, N = 41, L in {8, 40} in bf16 and f32; B = 4, N = 200, L = 40 in f32 -- and per call
    partition forward | partition forward + backward | marginals | tree_entropy with gradient | sample_heads with labels at S = 8
three things are timed in alternating windows of N replays, R times (the median and the spread of the repeats are kept):
  (a) the labeled call of this package (vlg_label_fold / _expand / _draw around the DP);
  (b) the unlabeled call on arc scores [B,N,N] of the same (B, N): what the DP alone costs (vlg_deptree_inside / _inside_outside /
      _expect / _sample);
  (c) the torch composite a user would write without (a): `phi.logsumexp(-1)` into the unlabeled call, autograd spreading the arc
      gradient over the labels (softmax * g); for the entropy, autograd through `expected_score`-free algebra is not available in
      the unlabeled path, so (c) is the value H = logZ - <mu, (softmax * phi).sum(-1)> with its forward only.  For the sampler
      (c) is the tree draw plus a torch.multinomial over the gathered rows.
fold and expand are also timed alone on full-length sentences, with the bytes they move (fold: the read cells of phi in, arc out;
expand: the read cells of phi, arc and g1 in, the whole gradient out in phi's type), the rate, and its share of the 6.29 TB/s streaming rate measured for this chip; registers and LDS per kernel come from
tools/codeobj.py.  Prints one JSON line per shape and writes the list to FILE (default profiles/deptree_labeled.json).
A machine without a GPU fails here: nothing is estimated."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch

from vlgae_amd import _C
from vlgae_amd.encoders import DeviceRng
from vlgae_amd.torch_struct import DependencyCRF
from vlgae_amd.torch_struct import functional as F

dev = torch.device('cuda:0')
arg = lambda name, default: ([a.split('=')[1] for a in sys.argv if a.startswith(f'--{name}=')] or [default])[0]
REPLAYS, REPEATS = int(arg('replays', 300)), int(arg('repeats', 5))
OUT = arg('out', os.path.join(ROOT, 'profiles', 'deptree_labeled.json'))
STREAM_PEAK = 6.29e12
SHAPES = ((256, 41, 8, 'bf16'), (256, 41, 8, 'f32'), (256, 41, 40, 'bf16'), (256, 41, 40, 'f32'), (4, 200, 40, 'f32'))
S = 8


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3): fn()
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fn()
    for _ in range(10): gr.replay()
    return gr


def window(gr, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): gr.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3     # us per replay


def timed(fns):
    "{name: {us, min, max}} of the callables, windows interleaved so that drift hits all alike"
    graphs, failed = {}, {}
    for k, f in fns.items():
        try:
            graphs[k] = graph_of(f)
        except Exception as e:             # (a composite that cannot be captured is reported, not guessed)
            failed[k] = f'not measured ({type(e).__name__}: {str(e).splitlines()[0][:120]})'
            torch.cuda.synchronize()
    runs = {k: [] for k in graphs}
    for _ in range(REPEATS):
        for k, g in graphs.items():
            runs[k].append(window(g, REPLAYS))
    out = {k: dict(us=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in runs.items()}
    out.update(failed)
    return out


def shape_record(B, N, L, dtype):
    dt = torch.bfloat16 if dtype == 'bf16' else torch.float32
    es = 2 if dtype == 'bf16' else 4
    g = torch.Generator(device=dev).manual_seed(B + N + L)
    phi = torch.randn((B, N, N, L), generator=g, device=dev).to(dt).requires_grad_(True)
    ln = torch.randint(N // 2, N, (B,), generator=g, device=dev)
    ln[0] = N - 1
    arc = torch.randn((B, N, N), generator=g, device=dev).to(dt).requires_grad_(True)
    rng = DeviceRng(7, dev)
    pos = torch.arange(N, device=dev)

    def torch_arc():
        return phi.logsumexp(-1)

    def torch_entropy():
        with torch.no_grad():
            a = phi.float().logsumexp(-1)
            pbar = (torch.softmax(phi.float(), -1) * phi.float()).sum(-1)
            lz, ev, _, _ = F.deptree_expect(a, ln, v=pbar)
            return lz - ev

    def torch_sample():
        with torch.no_grad():
            heads = DependencyCRF(phi.float().logsumexp(-1), ln).sample_heads(S, rng=rng)
            rows = phi.detach()[torch.arange(B, device=dev)[None, :, None], heads, pos[None, None, :]]      # [S,B,N,L]
            return heads, torch.multinomial(torch.softmax(rows.float(), -1).view(-1, L), 1).view(S, B, N)

    calls = {
        'partition': dict(labeled=lambda: DependencyCRF(phi.detach(), ln).partition, unlabeled=lambda: DependencyCRF(arc.detach(), ln).partition,
                          torch=lambda: DependencyCRF(torch_arc().detach(), ln).partition),
        'partition_backward': dict(labeled=lambda: torch.autograd.grad(DependencyCRF(phi, ln).partition.sum(), phi),
                                   unlabeled=lambda: torch.autograd.grad(DependencyCRF(arc, ln).partition.sum(), arc),
                                   torch=lambda: torch.autograd.grad(DependencyCRF(torch_arc(), ln).partition.sum(), phi)),
        'marginals': dict(labeled=lambda: DependencyCRF(phi.detach(), ln).marginals, unlabeled=lambda: DependencyCRF(arc.detach(), ln).marginals,
                          torch=lambda: torch.softmax(phi.detach().float(), -1) * DependencyCRF(torch_arc().detach(), ln).marginals.unsqueeze(-1)),
        'entropy_grad': dict(labeled=lambda: torch.autograd.grad(DependencyCRF(phi, ln).tree_entropy().sum(), phi),
                             unlabeled=lambda: torch.autograd.grad(DependencyCRF(arc, ln).tree_entropy().sum(), arc),
                             torch_forward_only=torch_entropy),
        f'sample_S{S}': dict(labeled=lambda: DependencyCRF(phi.detach(), ln).sample_heads(S, rng=rng, return_labels=True),
                             unlabeled=lambda: DependencyCRF(arc.detach(), ln).sample_heads(S, rng=rng), torch=torch_sample),
    }
    rec = dict(B=B, N=N, L=L, dtype=dtype, replays=REPLAYS, repeats=REPEATS, calls={k: timed(v) for k, v in calls.items()})
    # the two streaming kernels alone, on full-length sentences: every cell but child 0 and the diagonal is read
    with torch.no_grad():
        a, best, _ = F.label_fold(phi.detach(), None, 0)
        g1 = torch.rand((B, N, N), device=dev)
        alone = timed(dict(fold=lambda: F.label_fold(phi.detach(), None, 0), expand=lambda: F.label_expand(phi.detach(), None, 0, a, g1, out_dtype=dt)))
    rows, live = B * N * N, B * (N - 1) * (N - 1)
    moved = dict(fold=live * L * es + rows * 4, expand=live * L * es + rows * L * es + live * 8)   # phi in | arc out; phi, arc, g1 in | gradient out
    for k, v in alone.items():
        if not isinstance(v, dict):
            continue
        v['bytes'] = moved[k]
        v['TB_per_s'] = round(moved[k] / (v['us'] * 1e-6) / 1e12, 3)
        v['share_of_stream_peak'] = round(moved[k] / (v['us'] * 1e-6) / STREAM_PEAK, 3)
    rec['kernels_alone'] = alone
    rec['lanes_per_row'] = _C.lib().vlg_label_lanes(L, 1 if dtype == 'bf16' else 0) & 0xFF
    rec['vector_image'] = bool(_C.lib().vlg_label_lanes(L, 1 if dtype == 'bf16' else 0) & 0x100)
    return rec


def resources():
    "vgpr / sgpr / LDS / scratch of the three kernels' images, from the built object"
    try:
        import codeobj
        out = {}
        for k in codeobj.kernels_of(os.path.join(ROOT, 'vlgae_amd', '_lib', 'vlg_label.o')):
            name = k.get('demangled') or k.get('name')
            out[name] = {f: k.get(f) for f in ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'group_segment_fixed_size',
                                              'private_segment_fixed_size', 'max_flat_workgroup_size', 'text_bytes') if k.get(f) is not None}
        return out
    except Exception as e:                 # the object is not on this machine: say so instead of guessing
        return f'not read ({type(e).__name__}: {e})'


def main():
    if '--resources' in sys.argv:
        doc = json.load(open(OUT))
        doc['kernel_resources'] = resources()
        with open(OUT, 'w') as f:
            json.dump(doc, f, indent=1)
        print('wrote kernel_resources into', OUT)
        return
    assert torch.cuda.is_available(), 'time_labeled.py needs an MI355X'
    recs = []
    for shape in SHAPES:
        recs.append(shape_record(*shape))
        print(json.dumps(recs[-1]), flush=True)
    doc = dict(device=torch.cuda.get_device_name(0), stream_peak_TB_per_s=STREAM_PEAK / 1e12, shapes=recs, kernel_resources=resources())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        json.dump(doc, f, indent=1)
    print('wrote', OUT)


if __name__ == '__main__':
    main()
