"""taming KL-VAE oracle in torch on the CPU: the decoder, decode_latent (squares stitched along time), the encoder and quant_conv,
in float32 or float64, differentiable with autograd.

Test infrastructure (see oracle/__init__.py).  It restates oracle/vae_np.py (same functions, same state_dict keys, same config:
ch 128, ch_mult (1, 2, 2, 4), two ResnetBlocks per level, one attention in the middle, GroupNorm(32, eps 1e-6)) with the dtype as a
parameter, so that the float64 run is the reference of the input-family tests (tests/vae_cases.py) and the float32 run is the
arithmetic of the fp32 kernels.

Twin mode (`split` given, dtype float64): both operands of every conv and of every matrix product (3x3, 1x1, q.k^T, p.v) are rounded to
float32 and pass through the three-term split of csrc/common.h: hi = split_t(x), lo = split_t(x - hi), product hi*hi + hi*lo + lo*hi with
wide accumulation.  The backward products do the same with the incoming gradient as one operand.  Everything else (GroupNorm, swish,
softmax, bias, residual) stays in float64.  It restates the documented arithmetic of the bf16x3 modes, not the kernels.
`split` is a callable float32 ndarray -> (hi, lo) float64 ndarrays, e.g. tests/attn_cases.split_parts.

`hooks` (optional dict) swaps single operations for deliberately wrong ones: the mutants of tests/test_vae_cases_host.py; `probe`
(optional dict) collects what the family properties are asserted on (GroupNorm inputs, attention scores and probabilities)."""
import numpy as np
import torch
import torch.nn.functional as F

CH_MULT = (1, 2, 2, 4)
NUM_RES_BLOCKS = 2
GROUPS = 32
EPS = 1e-6


def _parts(x, split):
    hi, lo = split(x.detach().to(torch.float32).contiguous().numpy())
    return torch.from_numpy(hi), torch.from_numpy(lo)


class _X3Conv(torch.autograd.Function):
    """conv2d (no bias, no padding: the caller pads) of split operands; the input gradient is the same product with the split gradient"""

    @staticmethod
    def forward(ctx, x, w, stride, split):
        xp, wp = _parts(x, split), _parts(w, split)
        ctx.wp, ctx.stride, ctx.split, ctx.xshape = wp, stride, split, x.shape
        return F.conv2d(xp[0], wp[0] + wp[1], stride=stride) + F.conv2d(xp[1], wp[0], stride=stride)

    @staticmethod
    def backward(ctx, g):
        gp, wp = _parts(g, ctx.split), ctx.wp
        dx = torch.nn.grad.conv2d_input(ctx.xshape, wp[0] + wp[1], gp[0], stride=ctx.stride) \
            + torch.nn.grad.conv2d_input(ctx.xshape, wp[0], gp[1], stride=ctx.stride)
        return dx, None, None, None


class _X3Matmul(torch.autograd.Function):
    """a (.., m, k) @ b (.., k, n) of split operands; both gradients are split products as well"""

    @staticmethod
    def forward(ctx, a, b, split):
        ap, bp = _parts(a, split), _parts(b, split)
        ctx.ap, ctx.bp, ctx.split = ap, bp, split
        return ap[0] @ (bp[0] + bp[1]) + ap[1] @ bp[0]

    @staticmethod
    def backward(ctx, g):
        gp, ap, bp = _parts(g, ctx.split), ctx.ap, ctx.bp
        da = gp[0] @ (bp[0] + bp[1]).transpose(-1, -2) + gp[1] @ bp[0].transpose(-1, -2)
        db = (ap[0] + ap[1]).transpose(-1, -2) @ gp[0] + ap[0].transpose(-1, -2) @ gp[1]
        return da, db, None


class VAE:
    """sd: state dict of numpy arrays (or tensors) keyed like the checkpoint; dtype torch.float32 / torch.float64"""

    def __init__(self, sd, dtype=torch.float64, split=None, hooks=None, probe=None):
        assert split is None or dtype == torch.float64, "the twin runs in float64"
        self.dtype, self.split, self.hooks, self.probe = dtype, split, dict(hooks or {}), probe
        self.sd = {k: (v.detach().cpu() if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(dtype) for k, v in sd.items()}

    # ------------------------------------------------------------------------------------------- operations
    def conv(self, x, key, pad=(0, 0, 0, 0), stride=1):
        """pad = (left, right, top, bottom) zeros, like torch.nn.functional.pad"""
        w, b = self.sd[key + ".weight"], self.sd[key + ".bias"]
        if any(pad):
            x = self.hooks["pad"](x, pad, key) if "pad" in self.hooks else F.pad(x, pad)
        y = _X3Conv.apply(x, w, stride, self.split) if self.split is not None else F.conv2d(x, w, stride=stride)
        return y + b[None, :, None, None]

    def matmul(self, a, b):
        return _X3Matmul.apply(a, b, self.split) if self.split is not None else a @ b

    def groupnorm(self, x, key):
        m, c, h, w = x.shape
        g = x.reshape(m, GROUPS, -1)
        if self.probe is not None:
            self.probe.setdefault("gn_in", []).append((key, g.detach()))
        if "gn_stats" in self.hooks:
            mu, var = self.hooks["gn_stats"](g, key)
        else:
            mu = g.mean(-1, keepdim=True)
            var = ((g - mu) ** 2).mean(-1, keepdim=True)
        y = ((g - mu) / torch.sqrt(var + EPS)).reshape(m, c, h, w)
        return y * self.sd[key + ".weight"][None, :, None, None] + self.sd[key + ".bias"][None, :, None, None]

    @staticmethod
    def swish(x):
        return x * torch.sigmoid(x)

    def resnet_block(self, x, p):
        h = self.conv(self.swish(self.groupnorm(x, p + "norm1")), p + "conv1", (1, 1, 1, 1))
        h = self.conv(self.swish(self.groupnorm(h, p + "norm2")), p + "conv2", (1, 1, 1, 1))
        if p + "nin_shortcut.weight" in self.sd:
            x = self.conv(x, p + "nin_shortcut")
        return x + h

    def attn_block(self, x, p):
        m, c, h, w = x.shape
        hn = self.groupnorm(x, p + "norm")
        q, k, v = (self.conv(hn, p + n).reshape(m, c, h * w) for n in "qkv")
        s = self.matmul(q.transpose(1, 2), k) * (int(c) ** -0.5)            # (m, hw_q, hw_k)
        pr = self.hooks["softmax"](s) if "softmax" in self.hooks else torch.softmax(s, dim=-1)
        if self.probe is not None:
            self.probe.setdefault("scores", []).append((p, s.detach()))
            self.probe.setdefault("probs", []).append((p, pr.detach()))
        o = self.matmul(v, pr.transpose(1, 2)).reshape(m, c, h, w)          # o[c, i] = sum_j v[c, j] p[i, j]
        return x + self.conv(o, p + "proj_out")

    # ------------------------------------------------------------------------------------------- the networks
    def decode(self, z):
        """AutoencoderKL.decode: z (M, 4, 16, 16) -> (M, 3, 128, 128)"""
        d = "decoder."
        h = self.conv(self.conv(z.to(self.dtype), "post_quant_conv"), d + "conv_in", (1, 1, 1, 1))
        h = self.resnet_block(h, d + "mid.block_1.")
        h = self.attn_block(h, d + "mid.attn_1.")
        h = self.resnet_block(h, d + "mid.block_2.")
        for lvl in reversed(range(len(CH_MULT))):
            for ib in range(NUM_RES_BLOCKS + 1):
                h = self.resnet_block(h, f"{d}up.{lvl}.block.{ib}.")
            if lvl != 0:
                h = self.conv(h.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), f"{d}up.{lvl}.upsample.conv", (1, 1, 1, 1))
        h = self.swish(self.groupnorm(h, d + "norm_out"))
        return self.conv(h, d + "conv_out", (1, 1, 1, 1))

    def decode_latent(self, latent, scale_factor=1.0):
        """_decode: latent (N, 4, H, 16) / scale_factor -> roll (N, 3, 128, 8 H), one square per 16 latent rows, stitched along time"""
        k = latent.shape[2] // 16
        z = (latent.to(self.dtype) / scale_factor).permute(0, 1, 3, 2)
        roll = self.decode(torch.cat(torch.chunk(z, k, dim=-1), dim=0))
        return torch.cat(torch.chunk(roll, k, dim=0), dim=-1)

    def encode_moments(self, x):
        """AutoencoderKL.encode_save(x, range_fix=False): x (M, 3, 128, 128) -> moments (M, 8, 16, 16) = mean | logvar.
        The stride-2 convs pad one zero on the right and at the bottom only."""
        e = "encoder."
        h = self.conv(x.to(self.dtype), e + "conv_in", (1, 1, 1, 1))
        for lvl in range(len(CH_MULT)):
            for ib in range(NUM_RES_BLOCKS):
                h = self.resnet_block(h, f"{e}down.{lvl}.block.{ib}.")
            if lvl != len(CH_MULT) - 1:
                h = self.conv(h, f"{e}down.{lvl}.downsample.conv", (0, 1, 0, 1), stride=2)
        h = self.resnet_block(h, e + "mid.block_1.")
        h = self.attn_block(h, e + "mid.attn_1.")
        h = self.resnet_block(h, e + "mid.block_2.")
        h = self.swish(self.groupnorm(h, e + "norm_out"))
        return self.conv(self.conv(h, e + "conv_out", (1, 1, 1, 1)), "quant_conv")

    def decode_latent_vjp(self, latent, cot, scale_factor=1.0):
        """(roll, d(latent)) with d(latent) = (d roll / d latent)^T cot by autograd"""
        with torch.enable_grad():
            lat = latent.to(self.dtype).clone().requires_grad_(True)
            roll = self.decode_latent(lat, scale_factor)
            (g,) = torch.autograd.grad(roll, lat, cot.to(self.dtype))
        return roll.detach(), g
