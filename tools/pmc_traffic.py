#!/usr/bin/env python
"""Per-kernel HBM traffic from two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE; rocpd sqlite output).
usage: tools/pmc_traffic.py fetch.db write.db [out.md [out.json steps_profiled]]
(out.json: the layout-0 GEMM family's bytes per launch, read by bench.py for roofline.traffic)
Values are the tool's kilobyte counters per dispatch, averaged per kernel name.  gfx950 correction
(MI355X_MICROARCH.md, HBM section): FETCH_SIZE counts wide coalesced streaming reads at exactly half their bytes ->
doubled here; WRITE_SIZE is calibrated on kernels of this run with a known byte count (cast_kernel, adamw_kernel)."""
import re
import sqlite3
import sys


def load(path, counter):
    cur = sqlite3.connect(path).cursor()
    rows = cur.execute("select kernel_name, count(*), sum(value), sum(end-start) from counters_collection where counter_name=? "
                       "group by kernel_name", (counter,)).fetchall()
    return {r[0]: (r[1], r[2], r[3]) for r in rows}


def short(n):
    n = re.sub(r"\(.*", "", n)
    return n if len(n) < 80 else n[:77] + "..."


f = load(sys.argv[1], "FETCH_SIZE")
w = load(sys.argv[2], "WRITE_SIZE")
lines = ["| kernel | launches | FETCH_SIZE x2 MB/launch | WRITE_SIZE MB/launch | avg us (PMC run) |", "|---|---|---|---|---|"]
tot = {}
for k in sorted(f, key=lambda k: -(f[k][1] * 2 + w.get(k, (0, 0, 0))[1])):
    n, kb, ns = f[k]
    wn, wkb, _ = w.get(k, (n, 0.0, 0))
    tot[k] = (n, 2 * kb / n / 1024, wkb / max(wn, 1) / 1024)
    lines.append(f"| `{short(k)}` | {n} | {2 * kb / n / 1024:.2f} | {wkb / max(wn, 1) / 1024:.2f} | {ns / n / 1e3:.1f} |")
txt = "\n".join(lines[:42])
print(txt)
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write(txt + "\n")

if len(sys.argv) > 5:
    import json
    steps = int(sys.argv[5])
    fam = [k for k in f if re.search(r"gemm_(huge_|h192_|h192l_|big_|q_)?kernel<true, true|gemm_ps_kernel<", k)]
    n = sum(f[k][0] for k in fam)
    fb = sum(f[k][1] for k in fam) * 2 * 1024 / n
    wb = sum(w.get(k, (0, 0, 0))[1] for k in fam) * 1024 / n
    allf = sum(v[1] for v in f.values()) * 2 * 1024
    allw = sum(v[1] for v in w.values()) * 1024
    json.dump({"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) --kernel-trace -- python bench.py --steps 1 --warmup 1 --full --no-cpu-baseline --no-ref-loop",
               "kernel": "layout-0 GEMMs (gemm_ps/gemm_huge/h192/big/gemm_kernel<true,true,*>): forward x.W^T and input-gradient dy.(W^T)^T",
               "launches": n, "launches_per_step": n // steps, "fetch_bytes_per_launch": int(fb), "write_bytes_per_launch": int(wb),
               "hbm_bytes_per_launch": int(fb + wb), "step_fetch_GB": round(allf / steps / 1e9, 1), "step_write_GB": round(allw / steps / 1e9, 1),
               "corrections": "FETCH_SIZE x2 (gfx950: wide coalesced reads counted at half, MI355X_MICROARCH.md HBM section); WRITE_SIZE x1"},
              open(sys.argv[4], "w"), indent=1)
