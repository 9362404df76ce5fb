"""Validate a guidance classifier on a dataset under the reference's protocol: the forward_backward_log(prefix="val") of the reference's
scripts/classifier_train_aug.py under no-grad (docs/rounds/augment.md).

    python scripts/classifier_val.py --data_dir val.csv --model DiTRotary-S/8-cls --model_path CKPT --rule note_density
                                     [--pr_image_size 1024] [--batch_size 4] [--iterations 10] [--noised True] [--no_high_noise False]
                                     [--scale_factor 1.] [--outdir DIR] [--seed 0] [--synthetic_weights True]

Per batch: load_data (augmented on the device, labelled by the rule) -> VAE latents (get_KL) -> uniform t, folded by --no_high_noise ->
noised latents (one launch with the latent windows) -> classifier forward.  Losses as the reference: MSE averaged over the outputs for a
rule, cross-entropy and acc@1 on `y` without one, (CE_key + mean CE_chord) / 2 and the chords' acc@1 for chord_progression.
val_results.csv holds one row per batch, run_metadata.json the flags and the per-quartile means.  No gradients, no optimiser."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from guided_diffusion.script_util import add_dict_to_argparser, args_to_dict, create_diffusion, diffusion_defaults  # noqa: E402


def create_argparser():
    defaults = dict(data_dir="", model="DiTRotary-S/8-cls", model_path="", in_channels=4, noised=True, no_high_noise=False, iterations=10,
                    batch_size=4, encode_rep=1, get_KL=True, scale_factor=1., embed_model_name="kl/f8-all-onset",
                    embed_model_ckpt="taming-transformers/checkpoints/all_onset/epoch_14.ckpt", pr_image_size=1024, rule=None, num_classes=9,
                    schedule_sampler="uniform", outdir="", synthetic_weights=False, gemm_precision="bf16x3_presplit", seed=0)
    defaults.update(diffusion_defaults())
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_dict_to_argparser(parser, defaults)
    return parser


def build(args, device):
    """(classifier, diffusion, VAE or None) as the flags ask."""
    from guided_diffusion import dist_util
    from guided_diffusion.dit import DiT_models
    from load_utils import load_model
    latent_rows = 16 * args.pr_image_size // 128 if args.get_KL else 128
    width = 16 if args.get_KL else args.pr_image_size
    model = DiT_models[args.model](input_size=[latent_rows, width], in_channels=args.in_channels, num_classes=args.num_classes)
    if not hasattr(model, "chord"):
        raise ValueError(f"{args.model} is not a classifier")
    if args.synthetic_weights:
        from rgm import synth
        arch = dict(depth=model.depth, hidden=model.hidden_size, heads=model.num_heads, patch=model.patch_size, in_ch=args.in_channels,
                    classifier=True, cls_classes=args.num_classes, chord=model.chord)
        model.load_state_dict(synth.dit_state_dict(3, device=device, **arch))
    else:
        model.load_state_dict(dist_util.load_state_dict(args.model_path, map_location="cpu"))
    model.to(device)
    model.eval()
    diffusion = create_diffusion(**args_to_dict(args, list(diffusion_defaults())))
    embed_model = None
    if args.get_KL:
        embed_model = load_model(args.embed_model_name, None if args.synthetic_weights else args.embed_model_ckpt)
        if args.synthetic_weights:
            from rgm import synth
            embed_model.load_state_dict(synth.vae_state_dict(2, device=device, encoder=True))
        embed_model.to(device)
        embed_model.eval()
    return model, diffusion, embed_model


def labels_of(extra, rule, device):
    import torch as th
    if rule is None:
        return extra["y"].to(device)
    if rule == "chord_progression":
        key = th.as_tensor(extra["key"]).to(device).reshape(-1, 1)
        return th.concat((key, extra["chord"].to(device).long()), dim=-1)       # B x (1 + chords)
    return extra[rule].to(device)


def losses_of(model, x, t, labels, rule, prefix="val"):
    """The reference's per-sample losses of one batch: {prefix_loss [, prefix_acc@1]}."""
    import torch as th
    import torch.nn.functional as F
    out = {}
    if rule == "chord_progression":
        key, chord = model(x, t)
        chord = chord.reshape(-1, chord.shape[-1])
        labels_key, labels_chord = labels[:, 0], labels[:, 1:].reshape(-1)
        loss_key = F.cross_entropy(key, labels_key, reduction="none")
        loss_chord = F.cross_entropy(chord, labels_chord, reduction="none").reshape(x.shape[0], -1).mean(dim=-1)
        out[f"{prefix}_loss"] = ((loss_key + loss_chord) / 2).detach()
        out[f"{prefix}_acc@1"] = (chord.argmax(dim=-1) == labels_chord).float()
    elif rule is not None:
        logits = model(x, t)
        out[f"{prefix}_loss"] = F.mse_loss(logits, labels.to(logits.dtype), reduction="none").mean(dim=-1).detach()
    else:
        logits = model(x, t)
        out[f"{prefix}_loss"] = F.cross_entropy(logits, labels, reduction="none").detach()
        out[f"{prefix}_acc@1"] = (logits.argmax(dim=-1) == labels).float()
    return out


def main(argv=None):
    import numpy as np
    import torch as th
    from guided_diffusion import train_util
    from guided_diffusion.pr_datasets_all import load_data
    from guided_diffusion.resample import create_named_schedule_sampler, fold_high_noise
    from rgm import native as _native
    args = create_argparser().parse_args(argv)
    if not args.data_dir or args.iterations < 1 or args.encode_rep < 1 or args.batch_size // args.encode_rep < 1:
        raise ValueError("classifier_val: --data_dir, iterations >= 1 and batch_size >= encode_rep >= 1 are needed")
    if args.pr_image_size % 128 or args.pr_image_size < 128:
        raise ValueError(f"pr_image_size = {args.pr_image_size}: a multiple of 128")
    _native.set_gemm_precision(args.gemm_precision)
    th.manual_seed(args.seed)
    device = th.device("cuda", th.cuda.current_device())
    model, diffusion, embed_model = build(args, device)
    sampler = create_named_schedule_sampler(args.schedule_sampler, diffusion)
    sampler.rng = np.random.default_rng([args.seed, 1])
    data = load_data(data_dir=args.data_dir, batch_size=args.batch_size // args.encode_rep, class_cond=args.rule is None,
                     deterministic=False, image_size=args.pr_image_size, rule=args.rule, device=device,
                     rng=np.random.default_rng([args.seed, 0]))
    outdir = args.outdir or "."
    os.makedirs(outdir, exist_ok=True)
    sink, rows = {}, []
    with th.no_grad():
        for it in range(args.iterations):
            batch, extra = next(data)
            labels = labels_of(extra, args.rule, device)
            n = batch.shape[0]
            if args.noised:
                t, _ = sampler.sample(n, device)
                if args.no_high_noise:
                    t = fold_high_noise(t, diffusion.num_timesteps)
            else:
                t = th.zeros(n, dtype=th.long, device=device)
            if args.get_KL and args.noised:
                _, x = train_util.get_noised_kl_input(batch, t, diffusion, model=embed_model, scale_factor=args.scale_factor)
            elif args.get_KL:
                x = train_util.get_kl_input(batch, model=embed_model, scale_factor=args.scale_factor, recombine=False)
            else:
                x = diffusion.q_sample(batch, t) if args.noised else batch
            if x.shape[0] != labels.shape[0]:
                labels = labels.repeat_interleave(args.encode_rep, dim=0)
            losses = losses_of(model, x, t, labels, args.rule)
            train_util.log_loss_dict(diffusion, t, losses, sink=sink)
            row = {"iteration": it, "t": " ".join(str(int(v)) for v in t.cpu().numpy())}
            row.update({k: repr(float(v.float().mean().item())) for k, v in losses.items()})
            rows.append(row)
    with open(os.path.join(outdir, "val_results.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    meta = {k: getattr(args, k) for k in vars(args)}
    meta["means"] = train_util.logged_means(sink)
    with open(os.path.join(outdir, "run_metadata.json"), "w") as f:
        json.dump(meta, f, indent=1)
    return meta


if __name__ == "__main__":
    main()
