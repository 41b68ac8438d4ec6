"""Summarise rocprofv3 SQ/TCC counter passes (tools/pmc_one.sh) for the dominant render kernel of a config.

    python tools/sq_summary.py gpurun_out/sq_c2/pmc --kernel "pt_megakernel<false" --cycles-per-sec 2.4e9 \
        --ms 0.59 [--json out.json]

--kernel is a comma list of kernel name parts: a dispatch of any of them counts (a split render's whole frame is
"pt_megakernel<false,pt_mk_tail<,pt_tiny_head<,pt_tiny_tail").

Derived: VALU issue share = SQ_INSTS_VALU * 2 cycles / (SIMDs * kernel cycles) (MI355X_MICROARCH.md: a wave64 VALU
instruction issues over 2 cycles on the 32-lane SIMD; one wave alone issues at most one per 4); wave-cycle split (WAIT_ANY / WAIT_INST_ANY / ACTIVE_INST_ANY over WAVE_CYCLES);
L2 hit rate = TCC_HIT / (TCC_HIT + TCC_MISS).
"""
import argparse
import csv
import glob
import json
import os
from collections import defaultdict


def grid_size(row) -> float:
    """Work-items of a dispatch row of a rocprofv3 counter_collection.csv."""
    for k in ("Grid_Size", "Grid_Size_X"):
        if row.get(k):
            return float(row[k]) * float(row.get("Grid_Size_Y") or 1) * float(row.get("Grid_Size_Z") or 1) \
                if k == "Grid_Size_X" else float(row[k])
    raise SystemExit("counter CSV without a grid-size column (needed for --frame-grid)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--kernel", required=True)
    ap.add_argument("--launches-per-frame", type=float, default=1.0)
    ap.add_argument("--ms", type=float, required=True, help="average duration of one launch of the kernel")
    ap.add_argument("--cycles-per-sec", type=float, default=2.4e9)
    ap.add_argument("--simds", type=int, default=1024)
    ap.add_argument("--json", default=None)
    ap.add_argument("--build-id", default=None, help="wcpt_build_id() of the library the passes measured")
    ap.add_argument("--config", default=None, help="bench config the passes ran (bench.py reads sq_<config>.json)")
    ap.add_argument("--camera", default="still", help="bench.py --camera of the passes (still | orbit)")
    ap.add_argument("--kernel-id", type=int, default=None, help="wcpt kernel variant (0 megakernel, 2 wavefront)")
    ap.add_argument("--bound", default=None, choices=["valu_issue", "memory_latency"],
                    help="the binding resource bench.py's roofline prices against")
    ap.add_argument("--resource", default=None, help="one-line description of the binding resource")
    ap.add_argument("--source", default=None, help="where the passes came from (round, script, kernel time)")
    ap.add_argument("--frame-grid", type=int, default=0,
                    help="work-items of the kernel per frame: counters are then per FRAME, summed over the dispatches "
                         "and scaled by frame grid / dispatched grid (the frame overlap splits a megakernel frame into "
                         "two launches of half the tiles), and --ms is the frame's time")
    a = ap.parse_args()
    per = defaultdict(list)
    grid = defaultdict(float)
    for f in glob.glob(os.path.join(a.dir, "p*", "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if any(f in row.get("Kernel_Name", "") for f in a.kernel.split(",")):
                per[row["Counter_Name"]].append(float(row["Counter_Value"]))
                grid[row["Counter_Name"]] += grid_size(row) if a.frame_grid else 0.0
    if a.frame_grid:
        m = {k: sum(v) * a.frame_grid / grid[k] for k, v in per.items()}
    else:
        m = {k: sum(v) / len(v) for k, v in per.items()}
    out = {"kernel": a.kernel, "counters_per_launch": {k: round(v, 1) for k, v in sorted(m.items())}}
    cycles = a.ms * 1e-3 * a.cycles_per_sec
    if "SQ_INSTS_VALU" in m:
        out["valu_issue_share"] = round(m["SQ_INSTS_VALU"] * 2.0 / (a.simds * cycles), 3)
    if "SQ_WAVE_CYCLES" in m:
        w = m["SQ_WAVE_CYCLES"]
        out["wave_cycle_split"] = {k: round(m[c] / w, 3) for k, c in
                                   (("wait_any", "SQ_WAIT_ANY"), ("wait_inst_any", "SQ_WAIT_INST_ANY"),
                                    ("active_inst_any", "SQ_ACTIVE_INST_ANY")) if c in m}
    if "TCC_HIT_sum" in m and "TCC_MISS_sum" in m:
        out["l2_hit_rate"] = round(m["TCC_HIT_sum"] / max(1.0, m["TCC_HIT_sum"] + m["TCC_MISS_sum"]), 3)
    if "SQ_THREAD_CYCLES_VALU" in m and "SQ_ACTIVE_INST_VALU" in m:
        out["lane_utilisation_valu"] = round(m["SQ_THREAD_CYCLES_VALU"] / max(1.0, 64.0 * m["SQ_ACTIVE_INST_VALU"]), 3)
    out["launches_per_frame"] = 1.0 if a.frame_grid else a.launches_per_frame
    if a.frame_grid:
        out["per_frame"] = (f"counters_per_launch hold one frame's counts: the dispatches' sums x {a.frame_grid} "
                            f"work-items per frame / the work-items dispatched")
    for k in ("config", "camera", "bound", "resource", "source"):
        if getattr(a, k) is not None:
            out[k] = getattr(a, k)
    if a.kernel_id is not None:
        out["kernel_name_filter"] = out["kernel"]
        out["kernel"] = a.kernel_id
    if a.build_id:
        out["build_id"] = a.build_id
    print(json.dumps(out, indent=1))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
