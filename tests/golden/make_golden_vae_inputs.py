#!/usr/bin/env python3
"""Generate the VAE input-family fixture under tests/golden/ by IMPORTING the reference:  `python tests/golden/make_golden_vae_inputs.py`.

Runs only in the build container, like make_golden.py / make_golden_peaked.py, whose shims and RefVAE recipe (the reference's own Decoder
/ Encoder classes plus the two 1x1 convs around them) it reuses.  No GPU test imports this file or the reference.

Families, inputs and the measure are tests/vae_cases.py's (weights and inputs are rebuilt from seeds; only the seeds are stored).

    vae_inputs.npz (+ .part2.npz, ..., joined by conftest.load_golden; no file over 1 MiB)
        <family>.roll64 / .dlat64          one square (latent (1, 4, 16, 16)): the reference in float64, roll and d(latent) for a seeded cotangent
        <family>.h32.roll64 / .dlat64      two squares (N = 1, H = 32) for `offset` and `impulse`
        enc.<weights>.mom64                moments of the three roll families under base / offset / gain weights, float64
        <case>.err_fp32.<quantity>         block errors against float64 of the reference in float32
        <case>.err_bf16x3.<quantity>       block errors against float64 of the bf16x3 twin (oracle/vae_torch.py, split operands)
        base.h32.err_*                     errors only: what R_p of the two-square cases is calibrated on
        gain.h32.u8, base.u8               the reference's decode_sample_for_midi (float32) of the two-square `gain` latent and of the square `base` latent

Asserted here: the reference's float32 stays below vae_cases.CONDITIONING_LIMIT in every block of every case (a family beyond that is
ill conditioned and has to be retuned), and oracle/vae_torch.py in float64 matches the reference's float64 to 1e-9 norm-wise."""
import glob
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs ref_shims, imports the reference)
import vae_cases as vc  # noqa: E402  (tests/vae_cases.py)

SEEDS = {"seed": vc.SEED, "gain_seed": vc.GAIN_SEED, "z_seed": vc.Z_SEED, "cot_seed": vc.COT_SEED}
LIMIT = 1024 * 1024
PART_BYTES = 900 * 1024
ORACLE_TOL = 1e-9


def save(name, arrs):
    for old in glob.glob(os.path.join(HERE, name + ".part*.npz")):
        os.remove(old)
    small = {k: v for k, v in arrs.items() if np.asarray(v).nbytes < 4096}
    parts, size = [small], sum(np.asarray(v).nbytes for v in small.values())
    for k, v in arrs.items():
        if k in small:
            continue
        n = np.asarray(v).nbytes
        if size + n > PART_BYTES and size > 0:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += n
    for i, part in enumerate(parts):
        p = os.path.join(HERE, name + (".npz" if i == 0 else f".part{i + 1}.npz"))
        with zipfile.ZipFile(p, "w", zipfile.ZIP_STORED) as zf:       # np.savez's layout with a fixed time stamp: the files regenerate bit for bit
            for k, v in part.items():
                buf = io.BytesIO()
                np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
                zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
        assert os.path.getsize(p) < LIMIT, f"{p}: {os.path.getsize(p)} bytes"
        print(f"  wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB)")


class Ref:
    """the reference's modules with a family's weights, in one dtype"""

    def __init__(self, shell, sd, dtype):
        t = mg.tsd(sd)
        shell.decoder.load_state_dict({k[len("decoder."):]: v for k, v in t.items() if k.startswith("decoder.")}, strict=True)
        shell.encoder.load_state_dict({k[len("encoder."):]: v for k, v in t.items() if k.startswith("encoder.")}, strict=True)
        shell.pq.load_state_dict({"weight": t["post_quant_conv.weight"], "bias": t["post_quant_conv.bias"]})
        shell.qc.load_state_dict({"weight": t["quant_conv.weight"], "bias": t["quant_conv.bias"]})
        for m in (shell.decoder, shell.encoder, shell.pq, shell.qc):
            m.to(dtype)
        self.v, self.dtype = shell, dtype

    def decode(self, lat, cot):
        """the reference's _decode arithmetic (gaussian_diffusion.py: squares along time) with autograd for d(latent)"""
        with torch.enable_grad():
            lt = torch.from_numpy(lat).to(self.dtype).requires_grad_(True)
            k = lt.shape[2] // 16
            z = torch.cat(torch.chunk(lt.permute(0, 1, 3, 2), k, dim=-1), dim=0)
            roll = torch.cat(torch.chunk(self.v.decode(z), k, dim=0), dim=-1)
            (g,) = torch.autograd.grad(roll, lt, torch.from_numpy(cot).to(self.dtype))
        assert roll.dtype == self.dtype
        return {"roll": roll.detach().double().numpy(), "dlat": g.double().numpy()}

    def encode(self, x):
        with torch.no_grad():
            return self.v.encode_save(torch.from_numpy(x).to(self.dtype)).double().numpy()


def check(case, what, e32, own):
    print(f"    {case} {what}: reference float32 worst block {e32.max():.2e}; oracle float64 against the reference's {own:.1e}", flush=True)
    assert e32.max() <= vc.CONDITIONING_LIMIT, f"{case} {what}: the float32 reference is off by {e32.max():.2e} in a block: ill conditioned, retune the family"
    assert own <= ORACLE_TOL, (case, what, own)


def main():
    out = {k: np.array([v], dtype=np.int64) for k, v in SEEDS.items()}
    shell = mg.RefVAE(vc.SEED, encoder=True)
    base = vc.base_weights()
    assert all(np.array_equal(base[k], shell.sd[k]) for k in base)
    for fam in vc.DECODE_FAMILIES:
        sd = vc.weights(fam, base)
        for H in (16, 32):
            if H == 32 and fam not in vc.TWO_SQUARE_FAMILIES + ("base",):
                continue
            case = vc.case_key(fam, "roll", H)
            print(f"[{case}]", flush=True)
            lat, cot = vc.latent(fam, H), vc.cotangent(H)
            r64 = Ref(shell, sd, torch.float64).decode(lat, cot)
            r32 = Ref(shell, sd, torch.float32).decode(lat, cot)
            own = vc.run_decode(vc.model(sd, "ref64"), lat, cot)
            twin = vc.run_decode(vc.model(sd, "bf16x3"), lat, cot)
            for qn in ("roll", "dlat"):
                e32, etw = vc.block_err(r32[qn], r64[qn], qn), vc.block_err(twin[qn], r64[qn], qn)
                check(case, qn, e32, vc.rel(own[qn], r64[qn]))
                print(f"      twin worst block {etw.max():.2e}", flush=True)
                out[f"{case}.err_fp32.{qn}"], out[f"{case}.err_bf16x3.{qn}"] = e32, etw
                if not (fam == "base" and H == 32):
                    out[f"{case}.{qn}64"] = r64[qn]
    # the integer stage: the reference's decode_sample_for_midi (float32) of the two-square `gain` latent, whose roll leaves [-1, 1], and of
    # the one-square `base` latent -- a square latent is the one shape that function does not transpose
    for key, fam, H in (("gain.h32.u8", "gain", 32), ("base.u8", "base", 16)):
        Ref(shell, vc.weights(fam, base), torch.float32)
        u8 = mg.rmu.decode_sample_for_midi(torch.from_numpy(vc.latent(fam, H).copy()), embed_model=shell, scale_factor=1.0, threshold=-0.95).numpy()
        assert u8.shape == (1, 128, 8 * H, 3) and u8.dtype == np.uint8
        out[key] = u8
    x = vc.rolls()
    for wf in vc.ENCODE_WEIGHTS:
        case = vc.case_key(wf, "moments")
        print(f"[{case}]", flush=True)
        sd = vc.weights(wf, base)
        m64 = Ref(shell, sd, torch.float64).encode(x)
        m32 = Ref(shell, sd, torch.float32).encode(x)
        own = vc.run_encode(vc.model(sd, "ref64"), x)
        twin = vc.run_encode(vc.model(sd, "bf16x3"), x)
        e32, etw = vc.block_err(m32, m64, "moments"), vc.block_err(twin, m64, "moments")
        check(case, "moments", e32, vc.rel(own, m64))
        print(f"      twin worst block {etw.max():.2e}", flush=True)
        out[f"{case}.mom64"], out[f"{case}.err_fp32.moments"], out[f"{case}.err_bf16x3.moments"] = m64, e32, etw
    save("vae_inputs", out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
