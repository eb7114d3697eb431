"""Times brmi_texmips_build and brmi_texmips_build_alpha on a 2048 x 2048 texture with HIP events (profiles/texmips_cost.md); an argument names a file
that receives a copy of the lines printed."""
import ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import texmips_ref as T
from basicrenderer_amd import capi
lib = capi.brmi_lib()
dev = torch.device("cuda:0")
W = H = 2048
mips = T.full_mip_count(W, H)
offs, total = T.mip_offsets(W, H, mips)
rng = np.random.default_rng(3)
img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
table = torch.from_numpy(T.srgb_table()).to(dev)
scratch = torch.zeros(4, dtype=torch.uint8, device=dev)
stats = torch.zeros(mips * 260, dtype=torch.int32, device=dev)
scales = torch.zeros(mips, dtype=torch.float32, device=dev)
out = []
def desc(t, srgb):
    d = capi.TextureDesc(); d.texels, d.width, d.height, d.mipCount, d.format = t.data_ptr(), W, H, mips, srgb
    for l, o in enumerate(offs): d.mipOffset[l] = o
    return d
# sixteen copies of the chain so that a timed build does not find its source in the caches of the build before it (16 x 21.3 MiB > 256 MiB)
bufs = [torch.zeros(total * 4, dtype=torch.uint8, device=dev) for _ in range(16)]
for b in bufs: b[: W * H * 4] = torch.from_numpy(img.reshape(-1)).to(dev)
s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
def run(alpha, srgb, same):
    def one(b):
        d = desc(b, srgb)
        rc = lib.brmi_texmips_build_alpha(C.byref(d), table.data_ptr(), stats.data_ptr(), scales.data_ptr(), s) if alpha else lib.brmi_texmips_build(C.byref(d), table.data_ptr(), scratch.data_ptr(), 4, s)
        assert rc == 0, lib.brmi_last_error(None)
    for b in bufs: one(b)
    torch.cuda.synchronize()
    ts = []
    for k in range(48):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); one(bufs[0] if same else bufs[k % 16]); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts = np.array(ts)
    return np.median(ts), ts.min(), ts.max()
for alpha in (0, 1):
    for srgb in (0, 1):
        for same in (0, 1):
            med, lo, hi = run(alpha, srgb, same)
            out.append(f"{'alpha' if alpha else 'plain'} {'srgb' if srgb else 'linear'} {'same buffer (cache-warm)' if same else 'rotating 16 buffers'}: median {med:.1f} us, min {lo:.1f}, max {hi:.1f} (48 builds, one event pair each)")
# the host's loop on the same image (environment.box_mips), and what an empty event pair measures
from basicrenderer_amd.environment import box_mips
ts = []
for _ in range(3):
    t0 = time.perf_counter(); box_mips(img); ts.append(time.perf_counter() - t0)
out.append("host box_mips, same image: " + ", ".join(f"{t:.3f}" for t in ts) + " s")
ts = []
for _ in range(48):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); e1.record(); e1.synchronize(); ts.append(e0.elapsed_time(e1) * 1e3)
out.append(f"empty event pair: median {np.median(ts):.1f} us (the share of every figure above that is the events' own)")
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
print("\n".join(out))
