"""K4 (HBM pattern test) kernel rates against kernels doing the same memory traffic,
on one 4 GiB buffer, one process, interleaved rounds, medians:

  hbm_pattern_write          vs hipMemsetAsync
  hbm_pattern_verify         vs ntm_stream_read
  hbm_pattern_verify_invert  vs ntm_stream_copy   (bytes read + bytes written)

then the same kernel templates at 1 / 2 / 4 / 8 float4 per lane
(tools/experiments/hbm_pattern_variants.hip, compiled here into validation/build/),
which is how kWriteUnroll / kVerifyUnroll in ntm/hbm_pattern.hpp were chosen.
Results: profiles/hbm_memtest/README.md.

  python tools/hbm_pattern_rates.py [--out DIR] [--gib 4] [--rounds 9] [--no-variants]
"""
import argparse
import ctypes
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from nvidia_terraform_modules_amd.ops import _lib, build  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default="hbm_pattern_rates", help="directory for rates.json")
ap.add_argument("--gib", type=int, default=4)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--no-variants", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("hbm_pattern_rates needs an MI355X: rates are not measured on a CPU")

OUT = Path(args.out)
OUT.mkdir(parents=True, exist_ok=True)
GiB = 1 << 30
N = args.gib * GiB
ROUNDS, LAUNCHES = args.rounds, args.launches
dev = torch.device("cuda")
lib = _lib.lib()
hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]


def load_variants():
    so = build.BUILD / "libntm_hbm_variants.so"
    src = ROOT / "tools" / "experiments" / "hbm_pattern_variants.hip"
    build.BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run([build.hipcc(), *build.COMMON_FLAGS, "-shared", str(src), "-o", str(so)], check=True)
    v = ctypes.CDLL(str(so))
    v.k4v_write.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    v.k4v_verify.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                             ctypes.c_void_p, ctypes.c_void_p]
    return v


var = None if args.no_variants else load_variants()
buf = torch.empty(N // 4, dtype=torch.int32, device=dev)
dst = torch.empty(N // 4, dtype=torch.int32, device=dev)
sink = torch.zeros(8192, dtype=torch.float32, device=dev)
res = torch.zeros(16, dtype=torch.int64, device=dev); res[2] = -1
st = lambda: _lib.stream_handle()

def timed(fn, n=LAUNCHES):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n

def chk(rc): assert rc == 0, rc

results = {}
def pair(name, fa, fb, bytes_a, bytes_b, prep=None):
    ra, rb = [], []
    for f in (fa, fb):
        if prep: prep()
        timed(f, 2)                                   # warm-up
    for r in range(ROUNDS):
        order = ((fa, ra, bytes_a), (fb, rb, bytes_b)) if r % 2 == 0 else ((fb, rb, bytes_b), (fa, ra, bytes_a))
        for f, acc, nb in order:
            if prep: prep()
            acc.append(nb / timed(f) / 1e12)
    ma, mb = statistics.median(ra), statistics.median(rb)
    results[name] = {"k4_TBps": ra, "ref_TBps": rb, "k4_median": ma, "ref_median": mb, "ratio": ma / mb}
    print(f"{name:34s} k4 {ma:6.3f} TB/s  ref {mb:6.3f} TB/s  ratio {ma / mb:5.3f}  (k4 {min(ra):.3f}-{max(ra):.3f}, ref {min(rb):.3f}-{max(rb):.3f})", flush=True)

p = buf.data_ptr()
for pat, pn in ((0, "addr"), (1, "hash")):
    # shipping C ABI
    pair(f"write {pn} vs hipMemsetAsync", lambda: chk(lib.ntm_hbm_pattern_write(p, N, 0, pat, 1, 0, st())),
         lambda: chk(hip.hipMemsetAsync(p, 0x5A, N, st())), N, N)
    def wr(): chk(lib.ntm_hbm_pattern_write(p, N, 0, pat, 1, 0, st()))
    wr()
    pair(f"verify {pn} vs stream_read", lambda: chk(lib.ntm_hbm_pattern_verify(p, N, 0, pat, 1, 0, 0, res.data_ptr(), st())),
         lambda: chk(lib.ntm_stream_read(p, N, sink.data_ptr(), st())), N, N)
    # verify+invert flips the buffer each launch: alternate the expected polarity
    state = {"inv": 0}
    def vi():
        chk(lib.ntm_hbm_pattern_verify(p, N, 0, pat, 1, state["inv"], 1, res.data_ptr(), st()))
        state["inv"] ^= 1
    wr(); state["inv"] = 0
    pair(f"verify_invert {pn} vs stream_copy", vi,
         lambda: chk(lib.ntm_stream_copy(p, dst.data_ptr(), N, st())), 2 * N, 2 * N)
    torch.cuda.synchronize()
    raw = res.cpu().numpy().tobytes()
    assert int.from_bytes(raw[0:8], "little") == 0, "verify found bad words during timing"

# unroll variants of the same kernel templates, against the same references
if var is not None:
    print("--- unroll variants (pattern hash) ---", flush=True)
for U in ((1, 2, 4, 8) if var is not None else ()):
    pair(f"U={U} write hash vs memset", lambda: chk(var.k4v_write(U, p, N, 1, st())),
         lambda: chk(hip.hipMemsetAsync(p, 0x5A, N, st())), N, N)
    chk(var.k4v_write(U, p, N, 1, st()))
    pair(f"U={U} verify hash vs stream_read", lambda: chk(var.k4v_verify(U, p, N, 1, 0, res.data_ptr(), st())),
         lambda: chk(lib.ntm_stream_read(p, N, sink.data_ptr(), st())), N, N)
torch.cuda.synchronize()
raw = res.cpu().numpy().tobytes()
results["bad_words_during_timing"] = int.from_bytes(raw[0:8], "little")
results["device"] = torch.cuda.get_device_name(0)
(OUT / "rates.json").write_text(json.dumps(results, indent=1))
print("bad words during timing:", results["bad_words_during_timing"])
