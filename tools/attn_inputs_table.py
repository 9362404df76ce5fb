#!/usr/bin/env python3
"""The tables of docs/rounds/attn_inputs.md from one run of tests/test_gpu_attn_inputs.py with RGM_ATTN_REPORT set:

    RGM_ATTN_REPORT=report.jsonl python -m pytest tests/test_gpu_attn_inputs.py -m gpu -q
    python tools/attn_inputs_table.py report.jsonl > tables.md

One line per (family, shape, mode, quantity): the worst block (over samples, heads and, for d(qkv), the three components) of the float32
reference, of the kernels in the three arithmetics and of the bf16x3 twin, all against float64, and R_p of both arithmetics."""
import json
import sys
from collections import OrderedDict


def main(path):
    rows, models = OrderedDict(), []
    for line in open(path):
        r = json.loads(line)
        if r["mode"] == "model":
            models.append(r)
            continue
        key = (r["family"], r["shape"], r["mode"], r["quantity"])
        row = rows.setdefault(key, {})
        row[r["precision"]] = max(r["kernel"])
        row["ref32"] = max(r["ref32"])
        if r["precision"] != "fp32":
            row["twin"] = max(r["twin"])
            row["R_x3"] = r["R"]
        else:
            row["R_fp32"] = r["R"]

    def f(v):
        return "-" if v is None else f"{v:.1e}"
    print("| family | shape | mode | quantity | ref32 | fp32 kernel | bf16x3 twin | bf16x3 kernel | presplit kernel | R fp32 | R bf16x3 |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for (fam, shape, mode, qn), r in rows.items():
        print(f"| {fam} | {shape} | {mode} | {qn} | {f(r.get('ref32'))} | {f(r.get('fp32'))} | {f(r.get('twin'))} | {f(r.get('bf16x3'))} | "
              f"{f(r.get('bf16x3_presplit'))} | {r.get('R_fp32', 0):.2f} | {r.get('R_x3', 0):.2f} |")
    print()
    print("| model | H | precision | output | gradient | reference float32: output | gradient |")
    print("|---|---|---|---|---|---|---|")
    for r in models:
        print(f"| {r['family']} | {r['shape'][1:]} | {r['precision']} | {r['kernel'][0]:.2e} | {r['kernel'][1]:.2e} | {r['ref32'][0]:.2e} | {r['ref32'][1]:.2e} |")


if __name__ == "__main__":
    main(sys.argv[1])
