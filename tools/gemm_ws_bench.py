"""Cold-operand per-launch time of the bottlenecks' shallow-K 1x1 products (conv3 forward, conv1
dgrad accumulating into the residual gradient) on the generic implicit GEMM (cn_gemm_ws_mode 0) and
on the weight-stationary persistent kernel (mode 2): graph-timed over > 600 MB of distinct operand
sets, so every launch reads its operands from HBM as in the training step.

    python tools/gemm_ws_bench.py [modes, e.g. 0,2,0,2]

TB/s = algorithmic bytes (A + B + C, + the old C for read-add-store) / time."""
import sys
import torch
sys.path.insert(0, '.')
from cosnet_amd import _native as nv
from cosnet_amd import ops

dev = torch.device('cuda:0')
bf = torch.bfloat16
SHAPES = [
    ("l3 conv3 fwd", 28800, 1024, 256, 0),
    ("l3 conv1 dgrad", 14400, 1024, 256, 2),
    ("l3 fwd m14400", 14400, 1024, 256, 0),
    ("l4 conv3 fwd", 28800, 2048, 512, 0),
    ("l4 conv1 dgrad", 14400, 2048, 512, 2),
    ("l2 conv3 fwd", 28800, 512, 128, 0),
    ("l2 conv1 dgrad", 14400, 512, 128, 2),
    ("l1 conv3 fwd", 113408, 256, 64, 0),
    ("l1 conv1 dgrad", 56704, 256, 64, 2),
]


def gtime(fns, reps=3):
    for f in fns:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for f in fns:
            f()
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        for _ in range(reps):
            for f in fns:
                f()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (3 * reps * len(fns)) * 1e3


lib = nv.load()
modes = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [0, 2, 0, 2]
for name, m, n, k, cm in SHAPES:
    sets = []
    per = (m * k + n * k + m * n * (2 if cm else 1)) * 2
    while per * len(sets) < 600e6 and len(sets) < 48:
        a = torch.randn(m, k, device=dev).to(bf)
        b = (torch.randn(n, k, device=dev) * 0.05).to(bf)
        c = torch.zeros(m, n, device=dev, dtype=bf)
        sets.append(lambda a=a, b=b, c=c: ops.gemm(a, b, m, n, k, lda=k, ldb=k, out=c, ldc=n, c_mode=cm))
    line = "%-16s M=%6d N=%5d K=%4d cm%d sets=%2d %5.1f MB |" % (name, m, n, k, cm, len(sets), per / 1e6)
    for md in modes:
        lib.cn_gemm_ws_mode(md)
        t = gtime(sets)
        line += " m%d %6.1f us %4.2f TB/s |" % (md, t, per / t / 1e6)
    lib.cn_gemm_ws_mode(1)
    print(line, flush=True)
    del sets
    torch.cuda.empty_cache()
