#!/usr/bin/env python3
"""The table of docs/rounds/vae_inputs.md: worst block per family, quantity and precision for the float32 reference, the fp32 kernels, the
bf16x3 twin and the bf16x3 / pre-split kernels.

    RGM_VAE_REPORT=report.jsonl python -m pytest tests/test_gpu_vae_inputs.py -m gpu -q      # on the GPU box: one JSON line per check
    python tools/vae_inputs_table.py report.jsonl                                            # anywhere: the markdown table

The reference columns come with the report lines (the tests copy them from tests/golden/vae_inputs.npz); where one case was checked
more than once (the saving forward repeats the roll) the worst figure is kept."""
import json
import sys

COLUMNS = [("ref32", None, None), ("fp32 kernel", "fp32", "auto"), ("twin", None, None), ("bf16x3 kernel", "bf16x3", "auto"),
           ("pre-split kernel", "bf16x3_presplit", "auto"), ("pre-split, big tiles", "bf16x3_presplit", "big")]


def main(path):
    rows, order = {}, []
    for line in open(path):
        r = json.loads(line)
        key = (r["family"], r["quantity"], r["H"])
        if key not in rows:
            rows[key] = {}
            order.append(key)
        row = rows[key]
        row["ref32"] = r["ref32"]
        if r["precision"] != "fp32":
            row["twin"] = r["comparator"]
        col = (r["precision"], r["route"])
        row[col] = max(row.get(col, 0.0), r["kernel"])
        row[("bound",) + col] = r["bound"]
        row[("R", r["precision"])] = r["R"]
    print("| family | quantity | squares | " + " | ".join(c[0] for c in COLUMNS) + " | bound fp32 / bf16x3 / pre-split |")
    print("|---|---|---|" + "---|" * (len(COLUMNS) + 1))
    for key in sorted(order, key=lambda k: (k[1] != "roll", k[1] != "dlat", k[2], order.index(k))):
        row = rows[key]
        cells = []
        for name, prec, route in COLUMNS:
            v = row.get(name if prec is None else (prec, route))
            over = prec is not None and v is not None and v > row[("bound", prec, route)]
            cells.append("-" if v is None else f"{v:.1e}" + (" **over**" if over else ""))
        bounds = " / ".join(f"{row[('bound', p, 'auto')]:.1e}" if ("bound", p, "auto") in row else "-" for p in ("fp32", "bf16x3", "bf16x3_presplit"))
        print(f"| {key[0]} | {key[1]} | {'3 tiles' if key[1] == 'moments' else key[2] // 16} | " + " | ".join(cells) + f" | {bounds} |")
    print()
    seen = set()
    for key in order:
        for prec in ("fp32", "bf16x3"):
            tag = (key[1], key[2], prec)
            if tag not in seen and ("R", prec) in rows[key]:
                seen.add(tag)
                print(f"R_p {key[1]} H={key[2]} {prec}: {rows[key][('R', prec)]:.2f}")


if __name__ == "__main__":
    main(sys.argv[1])
