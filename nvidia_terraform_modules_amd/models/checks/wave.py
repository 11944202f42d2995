"""K12: the Job's wave data-path and special-function check."""
from __future__ import annotations

import time

import numpy as np
import torch

from ...ops import wave as w
from ._common import begin, verdict


def wave_check(device: torch.device, corrupt: str | None = None, seed: int = 0x4B3C, grid_per_cu: int = 2,
               max_launches: int = 8) -> dict:
    """K12, the Job's wave data-path and special-function check (``NTM_WAVE_CHECK=1``) on
    ``device``, in the Job's sequence: per family (lane, ldstr, valu) the reference kernel makes
    the expected table, then ``grid_per_cu`` workgroups per CU run the family against it, launch
    after launch until every CU ran it (``max_launches`` is a cap, not a retry); sfu: one digest
    per instruction and workgroup held to the majority's, then the distance of every result from
    the host's brackets. A workgroup whose digest is off is named by its CU, and a second, small
    launch (one workgroup on that CU, one on another) names the first input whose words differ.
    ``corrupt="lane"`` flips bit 10 of one result word of workgroup 0 before its compare;
    ``corrupt="sfu"`` makes every workgroup on one CU flip bit 10 of one v_exp_f32 word. Returns the Job's fields: ``wave_lane_bad``, ``wave_ldstr_bad``,
    ``wave_valu_bad``, ``wave_sfu_inconsistent``, ``wave_sfu_max_distance``,
    ``wave_sfu_beyond_bound``, ``wave_cus_covered``, ``wave_seconds``, and ``ok``, ``failures``."""
    if corrupt not in (None, "lane", "sfu"):
        raise ValueError("corrupt must be None, 'lane' or 'sfu'")
    o, device, gpu = begin(device)
    t_begin = time.perf_counter()
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    grid = grid_per_cu * cus
    seed = (seed + gpu) & 0xFFFFFFFF
    out = {"failures": [], "wave_lane_bad": 0, "wave_ldstr_bad": 0, "wave_valu_bad": 0, "wave_sfu_inconsistent": 0,
           "wave_sfu_max_distance": {}, "wave_sfu_beyond_bound": 0}
    covered = []

    def where(r, t):
        h = int(r["hw_id"])
        return (int(r["xcc_id"]) & 15, (h >> 13) & 7, (h >> 12) & 1, (h >> 8) & 15, int(r["simd"][(t // 64) & 3]) & 3)

    def sweep(family, inputs, layout, expected, on_bad, fault=None, fault_key=None):
        seen, recs_all = set(), []
        for launch in range(max_launches):
            recs = o.wave_sweep(family, inputs, layout, expected, grid,
                                fault_wg=fault_key if fault_key is not None else 0 if fault is not None and launch == 0 else None,
                                fault_index=fault or 0)
            recs_all.append(recs)
            for r in recs:
                if r["magic"] != 0x4B31324B:
                    out["failures"].append(f"gpu{gpu}: wave {family}: a workgroup wrote no record")
                    continue
                seen.add((int(r["xcc_id"]) & 15, int(r["hw_id"]) & 0xFF00))
                if r["bad"]:
                    out[f"wave_{family}_bad"] += int(r["bad"])
                    if not any(f.startswith(f"gpu{gpu}: wave {family}") for f in out["failures"]):
                        out["failures"].append(on_bad(r, (~int(r["first"])) & 0xFFFFFFFF))
            if len(seen) >= cus:
                break
        covered.append(len(seen))
        return np.concatenate(recs_all)

    lanes = np.arange(256)
    with torch.cuda.device(device):
        # lane
        x = w.wave_hash32(seed, 0, lanes // 64, 0, lanes % 64)
        y = w.wave_hash32(seed, 1, lanes // 64, 0, lanes % 64)
        din = o.wave_to_device(np.concatenate([x, y]), device)
        ops_list = w.wave_lane_ops()
        exp = torch.cat([o.wave_lane_reference_gpu(i, None, din[:256], din[256:]) for i in range(len(ops_list))])
        fault = (8 + 15 + 2) * 256 + 2 * 64 + 19 if corrupt == "lane" else None      # row_shr:3 bound_ctrl:0, wave 2 lane 19
        sweep("lane", din, None, exp,
              lambda r, i: w.wave_failure_message(gpu, "lane", w.wave_lane_op_name(ops_list[i // 256]), where(r, i % 256), "lane",
                                                  i % 64, int(r["expected"]), int(r["got"])), fault)
        # ldstr
        imgs, exps = [], []
        for f, bits in enumerate(w.WAVE_TR_BITS):
            img = np.zeros(16384, np.uint8)
            st = w.wave_sweep_stride(bits)
            img[:64 * st] = w.wave_make_image(bits, 64, st, (seed + f) & 0xFFFFFFFF)
            imgs.append(img)
            exps.append(o.wave_tr_read_reference_gpu(bits, torch.from_numpy(img[:64 * st].copy()).to(device), st))
        base = np.cumsum([0] + [e.numel() for e in exps])

        def ldstr_line(r, i):
            f = int(np.searchsorted(base, i, side="right")) - 1
            bits = w.WAVE_TR_BITS[f]
            return w.wave_failure_message(gpu, "ldstr", f"tr_b{bits} stride {w.wave_sweep_stride(bits)}", where(r, i % 256),
                                          "element", i - int(base[f]), int(r["expected"]), int(r["got"]))
        sweep("ldstr", o.wave_to_device(np.concatenate(imgs).view(np.uint32), device), None, torch.cat(exps), ldstr_line)
        # valu
        cv = w.wave_cvt_inputs(seed, 1024)
        t3 = np.arange(768)
        abc = w.wave_hash32(seed, 2 + t3 // 256, (t3 // 64) & 3, 0, t3 % 64)
        din = o.wave_to_device(np.concatenate([abc, cv, cv[::-1]]), device)
        n = len(cv)
        exp = torch.cat([o.wave_valu("bitop3", din[:256], din[256:512], din[512:768], reference=True).reshape(-1),
                         o.wave_valu("cvt_pk_bf16", din[768:768 + n], din[768 + n:], reference=True)])
        sweep("valu", din, [n], exp,
              lambda r, i: w.wave_failure_message(gpu, "valu", f"bitop3:0x{i // 256:02x}" if i < 65536 else "cvt_pk_bf16_f32",
                                                  where(r, i % 256), "element", i % 256 if i < 65536 else i - 65536,
                                                  int(r["expected"]), int(r["got"])))
        # sfu
        lists = [w.wave_sfu_inputs(op)[0] for op in range(7)]
        d_all = o.wave_to_device(np.concatenate(lists), device)
        counts = [len(v) for v in lists]
        fault_key, fault_index = None, 1000
        if corrupt == "sfu":     # the CU workgroup 0 of a first launch ran on
            fault_key = o.wave_cu_key(o.wave_sweep("sfu", d_all, counts, None, grid)[0])
        recs = sweep("sfu", d_all, counts, None, None, fault=fault_index if fault_key is not None else None, fault_key=fault_key)
        recs = recs[recs["magic"] == 0x4B31324B]
        for op, name in enumerate(w.WAVE_SFU_OPS):
            vals, counts = np.unique(recs["digest"][:, op], return_counts=True)
            want = vals[np.argmax(counts)]
            off = recs[recs["digest"][:, op] != want]
            out["wave_sfu_inconsistent"] += len(off)
            if len(off) and not any(" sfu " in f for f in out["failures"]):
                wh, key = where(off[0], 0), o.wave_cu_key(off[0])
                line = (f"gpu{gpu}: wave sfu {name}: xcd {wh[0]} se {wh[1]} sh {wh[2]} cu {wh[3]}: digest "
                        f"{int(off[0]['digest'][op]):#x} differs from {int(want):#x} of the other workgroups (not seen again in "
                        "a second launch)")
                dx = o.wave_to_device(lists[op], device)
                there = o.wave_sfu_locate(op, dx, key, True, grid, max_launches, fault_key, fault_index)
                there = there and (there[0].cpu().numpy().view(np.uint32), there[1])
                other = o.wave_sfu_locate(op, dx, key, False, grid, max_launches, fault_key, fault_index)
                if there and other:
                    good = other[0].cpu().numpy().view(np.uint32)
                    diff = np.flatnonzero(good != there[0])
                    if len(diff):
                        i = int(diff[0])
                        wh = where(there[1], i % 256)
                        line = (f"gpu{gpu}: wave sfu {name}: xcd {wh[0]} se {wh[1]} sh {wh[2]} cu {wh[3]} simd {wh[4]} element {i} "
                                f"input 0x{int(lists[op][i]):08x}: expected 0x{int(good[i]):08x}, got 0x{int(there[0][i]):08x}, "
                                f"bad bits 0x{int(good[i]) ^ int(there[0][i]):08x}")[:199]
                out["failures"].append(line)
            dx = o.wave_to_device(lists[op], device)
            d = o.wave_sfu_distance(op, dx, o.wave_sfu(op, dx), w.WAVE_SFU_BOUND[name])
            out["wave_sfu_max_distance"][name] = {"d": d["max_d"], "judged": w.WAVE_SFU_BOUND[name] is not None,
                                                  "input": f"0x{int(lists[op][d['max_index']]) if d['max_d'] else 0:08x}"}
            if w.WAVE_SFU_BOUND[name] is not None and d["beyond"]:
                out["wave_sfu_beyond_bound"] += d["beyond"]
                out["failures"].append(f"gpu{gpu}: wave sfu {name}: {d['beyond']} result(s) beyond {w.WAVE_SFU_BOUND[name]} "
                                       f"step(s) of the bracket, first input 0x{int(lists[op][d['first_beyond']]):08x}")
    out["wave_cus_covered"] = min(covered)
    if out["wave_cus_covered"] < cus:
        out["failures"].append(f"gpu{gpu}: wave coverage: {cus - out['wave_cus_covered']} of {cus} CUs did not run every "
                               f"family after {max_launches} launches")
    return verdict(out, t_begin, "wave_seconds")
