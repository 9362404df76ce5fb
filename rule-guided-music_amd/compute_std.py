"""The latent scale_factor of a dataset: 1 / std of the VAE latents of augmented training batches -- the reference's compute_std.py with
flags in place of its constants (docs/rounds/augment.md).

    python compute_std.py --data_dir train.csv [--image_size 1024] [--batch_size 32] [--total_batch 256]
                          [--vae kl/f8-all-onset] [--vae_path CKPT | --synthetic_weights True] [--outdir .] [--seed N]

total_batch batches come from load_data (augmented on the device), go through the encoder, and their unscaled latents are collected on
the device; rgm_latent_std (csrc/augment.hip) takes the unbiased standard deviation of all their elements in float64.  Prints
`scale_factor: <value>` like the reference and writes it to run_metadata.json."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from guided_diffusion.script_util import str2bool  # noqa: E402


def create_argparser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--data_dir", required=True, type=str, help="csv with a midi_filename column of uint8 .npy excerpts")
    p.add_argument("--image_size", type=int, default=1024)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--total_batch", type=int, default=256, help="batches the statistic is taken over")
    p.add_argument("--vae", type=str, default="kl/f8-all-onset")
    p.add_argument("--vae_path", type=str, default="taming-transformers/checkpoints/all_onset/epoch_14.ckpt")
    p.add_argument("--synthetic_weights", type=str2bool, default=False, help="seeded encoder weights in place of the checkpoint")
    p.add_argument("--outdir", type=str, default=".", help="where run_metadata.json goes")
    p.add_argument("--seed", type=int, default=None, help="seed of the augmentation draws")
    return p


def latent_std(x):
    """(mean, unbiased std, 1 / std) of every element of the float32 device tensor x, as float64 numbers: two launches, one read."""
    import torch
    from rgm import native as _rgm
    _rgm.require_cuda(x)
    x = x.float().contiguous()
    n = x.numel()
    need = int(_rgm.lib.rgm_latent_std_workspace(n))
    if need == 0:
        raise ValueError(f"the latent statistic takes 1 .. 2^40 elements, got {n}")
    ws = torch.empty(need // 8, dtype=torch.float64, device=x.device)
    out = torch.empty(3, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _rgm.check(_rgm.lib.rgm_latent_std(_rgm.ptr(x), n, _rgm.ptr(out), _rgm.ptr(ws), need, _rgm.current_stream()))
    return tuple(float(v) for v in out.cpu().numpy())


def collect_latents(args, device):
    """The unscaled latents of total_batch augmented batches, (total_batch * batch_size, 4, 16 image_size / 128, 16) on the device."""
    import numpy as np
    import torch
    from guided_diffusion.pr_datasets_all import load_data
    from guided_diffusion.train_util import get_kl_input
    from load_utils import load_model
    embed_model = load_model(args.vae, None if args.synthetic_weights else args.vae_path)
    if args.synthetic_weights:
        from rgm import synth
        embed_model.load_state_dict(synth.vae_state_dict(2, device=device, encoder=True))
    embed_model.to(device)
    embed_model.eval()
    data = load_data(data_dir=args.data_dir, batch_size=args.batch_size, class_cond=False, deterministic=False, image_size=args.image_size,
                     device=device, rng=np.random.default_rng(args.seed))
    z = []
    with torch.no_grad():
        for _ in range(args.total_batch):
            batch, _ = next(data)
            z.append(get_kl_input(batch, model=embed_model, scale_factor=1., recombine=False))
    return torch.concat(z, dim=0)


def main(argv=None):
    import torch
    args = create_argparser().parse_args(argv)
    if args.total_batch < 1 or args.batch_size < 1:
        raise ValueError("compute_std: total_batch >= 1 and batch_size >= 1 are needed")
    device = torch.device("cuda", torch.cuda.current_device())
    latents = collect_latents(args, device)
    mean, std, scale_factor = latent_std(latents)
    print(f"scale_factor: {scale_factor}")
    print("done")
    meta = {"data_dir": args.data_dir, "image_size": args.image_size, "batch_size": args.batch_size, "total_batch": args.total_batch,
            "vae": args.vae, "synthetic_weights": bool(args.synthetic_weights), "seed": args.seed, "elements": latents.numel(),
            "mean": mean, "std": std, "scale_factor": scale_factor}
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "run_metadata.json"), "w") as f:
        json.dump(meta, f, indent=1)
    return meta


if __name__ == "__main__":
    main()
