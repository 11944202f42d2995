"""K6 (host-link check) rates on one MI355X: the push / pull kernels' knobs against
hipMemcpyAsync on the same pinned and HBM buffers, one process, the candidates
interleaved, medians over the rounds:

  sweep   blocks x U (16-byte vectors per lane and tile) x nontemporal or default accesses,
          push (device->host) and pull (host->device), with hipMemcpyAsync both ways as
          two more candidates of every round; the margin for "parity" is the spread
          (max - min) of the hipMemcpyAsync rates over the rounds themselves
  default the shipped configuration, the duplex rate (push one half, pull the other, two
          streams) and the chase latency (1024 slots, 4096 hops)
  job     amdgpu-validate --host-link-mib: the stage's seconds split into pinning,
          transfers and teardown, and the link state it read under load
  ab      the verdict time with the flag off against another binary (--parent-bin),
          runs interleaved

This is how kPushUnroll / kPullUnroll / the nontemporal flags (ntm/host_link.hpp) and
kPushBlocks / kPullBlocks (ntm/host_link_plan.hpp) were chosen. Results: profiles/host_link/README.md.

  python tools/host_link_rates.py [--out DIR] [--mib 256] [--rounds 7] [--parent-bin PATH]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nvidia_terraform_modules_amd import ops  # noqa: E402
from nvidia_terraform_modules_amd.ops import reference  # noqa: E402
from nvidia_terraform_modules_amd.ops.gpu import hbm_pattern, host_link  # noqa: E402

BIN = ROOT / "validation" / "build" / "amdgpu-validate"
BLOCKS = (16, 32, 64, 128, 256, 512, 1024, 2048)
SEED = 0x4B36


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def run_job(binary, *args):
    t0 = time.perf_counter()
    p = subprocess.run([str(binary), "--gpus", "1", "--size", "8192", "--json", *args],
                       capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit(f"{binary} {' '.join(args)} exited {p.returncode}: {p.stdout[-400:]} {p.stderr[-400:]}")
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    return rep, wall


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="host_link_rates", help="directory for rates.json / rates.log")
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-bin", default="")
    ap.add_argument("--ab-runs", type=int, default=7)
    ap.add_argument("--no-job", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("host_link_rates needs an MI355X: rates are not measured on a CPU")
    if a.rounds < 5:
        sys.exit("at least 5 rounds")
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    log = []

    def say(line=""):
        print(line, flush=True)
        log.append(line)

    n = a.mib << 20
    host = torch.empty(n // 4, dtype=torch.int32, pin_memory=True)
    dbuf = torch.empty(n // 4, dtype=torch.int32, device="cuda")
    res = hbm_pattern.new_pattern_result("cuda")
    ops.host_link_push(host, 1, seed=SEED)
    torch.cuda.synchronize()

    # ---- the sweep: every candidate once per round, in one fixed order
    cands = {}
    for nt in (1, 0):
        for u in host_link.HOST_LINK_UNROLLS:
            for b in BLOCKS:
                cfg, tag = (u, nt), f"b{b}_u{u}_{'nt' if nt else 'plain'}"
                cands["push_" + tag] = lambda b=b, cfg=cfg: ops.host_link_push(
                    host, 1, seed=SEED, blocks=b, config=cfg)
                cands["pull_" + tag] = lambda b=b, cfg=cfg: ops.host_link_pull(
                    host, 1, seed=SEED, blocks=b, config=cfg, result=res)
    cands["push_memcpy"] = lambda: host.copy_(dbuf, non_blocking=True)      # device->host
    cands["pull_memcpy"] = lambda: dbuf.copy_(host, non_blocking=True)      # host->device
    dbuf.copy_(host)
    for fn in cands.values():                                               # warm-up: load every code object
        fn()
    torch.cuda.synchronize()
    gbps = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():
            gbps[k].append(n / (event_ms(fn) * 1e-3) / 1e9)
    bad = hbm_pattern.read_pattern_result(res)
    med = {k: statistics.median(v) for k, v in gbps.items()}
    report = {"mib": a.mib, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
              "pull_bad_words_over_the_sweep": bad.bad_words,
              "sweep_median_GBps": med, "sweep_GBps": gbps}
    say(f"{torch.cuda.get_device_name(0)}; {a.mib} MiB, {a.rounds} rounds, medians in GB/s; "
        f"bad words over all pulls: {bad.bad_words}")
    for d in ("push", "pull"):
        ref = gbps[d + "_memcpy"]
        say(f"{d}: hipMemcpyAsync median {med[d + '_memcpy']:.2f} (min {min(ref):.2f}, max {max(ref):.2f}, "
            f"spread {max(ref) - min(ref):.2f})")
        for nt in ("nt", "plain"):
            say(f"  {nt:5s}  blocks " + " ".join(f"{b:7d}" for b in BLOCKS))
            for u in host_link.HOST_LINK_UNROLLS:
                say(f"         U={u}    " + " ".join(f"{med[f'{d}_b{b}_u{u}_{nt}']:7.2f}" for b in BLOCKS))
        best = max((k for k in med if k.startswith(d + "_b")), key=med.get)
        say(f"  best {best} {med[best]:.2f} = {med[best] / med[d + '_memcpy']:.3f} of hipMemcpyAsync")
        report[d + "_best"] = best

    # ---- the shipped defaults, duplex and the chase
    half = n // 2
    lo, hi = host[: half // 4], host[half // 4:]
    side = torch.cuda.Stream()
    shipped = {"push": [], "pull": [], "push_memcpy": [], "pull_memcpy": [], "duplex": []}

    def duplex():
        ops.host_link_push(lo, 1, seed=SEED)
        with torch.cuda.stream(side):
            ops.host_link_pull(hi, 1, seed=SEED, base=half, result=res)

    ops.host_link_push(host, 1, seed=SEED)
    for _ in range(a.rounds):
        shipped["push"].append(n / (event_ms(lambda: ops.host_link_push(host, 1, seed=SEED)) * 1e-3) / 1e9)
        shipped["pull"].append(n / (event_ms(lambda: ops.host_link_pull(host, 1, seed=SEED, result=res)) * 1e-3) / 1e9)
        shipped["push_memcpy"].append(n / (event_ms(cands["push_memcpy"]) * 1e-3) / 1e9)
        shipped["pull_memcpy"].append(n / (event_ms(cands["pull_memcpy"]) * 1e-3) / 1e9)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        duplex()
        torch.cuda.synchronize()
        shipped["duplex"].append(2 * half / (time.perf_counter() - t0) / 1e9)
    bad = hbm_pattern.read_pattern_result(res)
    table = reference.host_link_chase_table(1024, SEED)
    slots = torch.from_numpy(table.view(np.int64).reshape(-1).copy()).pin_memory()
    want, _ = reference.host_link_chase(slots, 4096)
    chase = [ops.host_link_chase(slots, 4096) for _ in range(a.rounds)]
    report["shipped"] = {"push_blocks": ops.host_link_default_blocks(),
                         "pull_blocks": ops.host_link_default_blocks(pull=True),
                         "push_tile_bytes": ops.host_link_tile_bytes(),
                         "pull_tile_bytes": ops.host_link_tile_bytes(pull=True),
                         "GBps": shipped, "median_GBps": {k: statistics.median(v) for k, v in shipped.items()},
                         "bad_words": bad.bad_words, "chase_final_ok": all(c[0] == want for c in chase),
                         "chase_ns_per_hop": [c[1] for c in chase]}
    say()
    say(f"shipped: blocks {ops.host_link_default_blocks()} / {ops.host_link_default_blocks(pull=True)}, tile {ops.host_link_tile_bytes()} / "
        f"{ops.host_link_tile_bytes(pull=True)} bytes (push / pull); bad words {bad.bad_words}")
    for k, v in shipped.items():
        say(f"  {k:12s} median {statistics.median(v):7.2f}  min {min(v):7.2f}  max {max(v):7.2f}")
    ns = [c[1] for c in chase]
    say(f"  chase        median {statistics.median(ns):7.0f} ns per hop (min {min(ns):.0f}, max {max(ns):.0f}); "
        f"final index ok: {all(c[0] == want for c in chase)}")
    del host, dbuf, slots
    torch.cuda.empty_cache()

    # ---- the Job: what the stage costs, what it read from sysfs, flag off against the parent
    if not a.no_job and BIN.exists():
        runs = [run_job(BIN, "--host-link-mib", str(a.mib)) for _ in range(3)]
        g = [r[0]["gpus"][0] for r in runs]
        report["job"] = [{k: v for k, v in x.items() if k.startswith("host_link")} for x in g]
        report["job_wall_s"] = [r[1] for r in runs]
        say()
        say(f"job --host-link-mib {a.mib} (3 runs, medians): stage "
            f"{statistics.median(x['host_link_s'] for x in g):.3f} s = pin "
            f"{statistics.median(x['host_link_pin_s'] for x in g):.3f} + transfers "
            f"{statistics.median(x['host_link_transfer_s'] for x in g):.3f} + teardown "
            f"{statistics.median(x['host_link_free_s'] for x in g):.3f}")
        for k in ("host_link_h2d_GBps", "host_link_d2h_GBps", "host_link_h2d_copy_GBps",
                  "host_link_d2h_copy_GBps", "host_link_duplex_GBps", "host_link_read_latency_us"):
            say(f"  {k:28s} " + " ".join(f"{x[k]:8.2f}" for x in g))
        say(f"  host_link_pcie under load: {json.dumps(g[-1]['host_link_pcie'])}")
        if a.parent_bin:
            ab = {"parent": [], "new": []}
            for i in range(a.ab_runs):
                order = [("parent", a.parent_bin), ("new", BIN)]
                for name, b in (order if i % 2 == 0 else order[::-1]):
                    rep, _ = run_job(b)
                    ab[name].append(rep["phases_s"]["end"])
            report["flag_off_verdict_s"] = ab
            say(f"flag off, verdict seconds over {a.ab_runs} interleaved runs: parent median "
                f"{statistics.median(ab['parent']):.3f} (min {min(ab['parent']):.3f}, max {max(ab['parent']):.3f}); "
                f"new median {statistics.median(ab['new']):.3f} (min {min(ab['new']):.3f}, max {max(ab['new']):.3f})")
    (out / "rates.json").write_text(json.dumps(report, indent=1) + "\n")
    (out / "rates.log").write_text("\n".join(log) + "\n")


if __name__ == "__main__":
    main()
