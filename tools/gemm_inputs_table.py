#!/usr/bin/env python3
"""The per-case table of docs/rounds/gemm_inputs.md: worst 16 x 16 block per family, shape and epilogue for the comparators and the kernels.

    RGM_GEMM_REPORT=report.jsonl python -m pytest tests/test_gpu_gemm_inputs.py -m gpu -q      # on the GPU box: one JSON line per check
    python tools/gemm_inputs_table.py report.jsonl                                             # anywhere: the markdown table

A row is (shape, epilogue, family); a kernel column keeps the worst figure over its tiles and names the tile and the (row tile, column tile)
it was found in.  The comparator columns come with the report lines.  LayerNorm cases (shape lnD) report rows instead of blocks."""
import json
import sys

PRECISIONS = ("fp32", "bf16x3", "bf16x3_presplit")


def main(path):
    rows, order = {}, []
    for line in open(path):
        r = json.loads(line)
        key = (r["shape"], tuple(r["epilogue"]), r["family"])
        if key not in rows:
            rows[key] = {}
            order.append(key)
        row = rows[key]
        p = r["precision"]
        row[("cmp", p)], row[("bound", p)], row[("R", p)] = r["comparator"], r["bound"], r["R"]
        if r["kernel"] >= row.get(("kernel", p), (-1.0,))[0]:
            row[("kernel", p)] = (r["kernel"], r["tile"], r["out_split"], r["row_tile"], r["col_tile"])
        row[("n", p)] = row.get(("n", p), 0) + 1
    print("| shape | epilogue | family | ref32 | fp32 kernels | twin | bf16x3 kernels | pre-split kernels (worst tile) | bound fp32 / bf16x3 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for key in order:
        row = rows[key]
        cells = []
        for p in PRECISIONS:
            if p != "bf16x3_presplit":
                cells.append(f"{row[('cmp', p)]:.1e}" if ("cmp", p) in row else "-")
            k = row.get(("kernel", p))
            if k is None:
                cells.append("-")
                continue
            over = " **over**" if k[0] > row[("bound", p)] else ""
            where = f" (tile {k[1]}{', split' if k[2] else ''} @ {k[3]},{k[4]}; {row[('n', p)]} runs)" if p == "bf16x3_presplit" else ""
            cells.append(f"{k[0]:.1e}{where}{over}")
        bounds = " / ".join(f"{row[('bound', p)]:.1e}" if ("bound", p) in row else "-" for p in ("fp32", "bf16x3_presplit"))
        print(f"| {key[0]} | {' '.join(map(str, key[1]))} | {key[2]} | " + " | ".join(cells) + f" | {bounds} |")
    print()
    seen = set()
    for key in order:
        for p in ("fp32", "bf16x3_presplit"):
            tag = (key[0], key[1], p)
            if tag not in seen and ("R", p) in rows[key]:
                seen.add(tag)
                print(f"R {key[0]} [{' '.join(map(str, key[1]))}] {p}: {rows[key][('R', p)]:.2f}")


if __name__ == "__main__":
    main(sys.argv[1])
