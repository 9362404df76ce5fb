"""Rule-guided sampling CLI -- same flags, YAML schema and outputs as the reference's scripts/sample_rule.py
(:40-314): builds the eps-network, the diffusion, the VAE and the guidance classifiers, turns the YAML's
target rules into model_kwargs, samples batches with DDPM / stochastic DDIM (+ classifier guidance and/or SCG,
+ DiffCollage for long sequences), decodes to uint8 piano rolls and reports per-rule losses in results.csv /
summary.csv.  Run from this directory's parent (rule-guided-music_amd/) exactly like the reference:

    python scripts/sample_rule.py --config_path scripts/configs/cond_demo/demo2.yml --model DiTRotary_XL_8 \
        --model_path <ema.pt> --vae_path <vae.ckpt> --image_size 128 16 --in_channels 4 --scale_factor 1.2465 \
        --class_cond True --num_classes 3 --class_label 1 --batch_size 4 --num_samples 20

Multi-GPU: `torchrun --nproc-per-node 8 scripts/sample_rule.py ...` shards the SCG candidates over the ranks
(RCCL all-gather of the rule log-probs); rank 0 writes the outputs.  --synthetic_weights skips the checkpoint
files (no network here) and uses rgm.synth weights: for smoke runs and benchmarking only.
"""
import argparse
import os
import sys
from functools import partial

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch as th  # noqa: E402

from guided_diffusion import dist_util, midi_util, logger  # noqa: E402
from guided_diffusion.dit import DiT_models  # noqa: E402
from guided_diffusion.script_util import (  # noqa: E402
    NUM_CLASSES, model_and_diffusion_defaults, create_diffusion, add_dict_to_argparser, args_to_dict, str2bool)
from guided_diffusion.gaussian_diffusion import _extract_rule  # noqa: E402
from guided_diffusion.condition_functions import model_fn, dc_model_fn, composite_nn_zt, composite_rule  # noqa: E402
from load_utils import load_model  # noqa: E402
import diff_collage as dc  # noqa: E402


KEEP_FLOAT_ROLLS = None   # tests only: a list -> main() appends every batch's FLOAT decoded roll (B,3,128,T) next to the uint8 one
NOISE_FN = None     # tests only: callable(shape, device) -> tensor installed as diffusion.noise_fn (teacher-forced parity runs)


DROPPED_RULES = []    # what setup_chord_backend removed under --skip_chord_rules (run_metadata.json, output directory suffix)


def setup_chord_backend(args, config):
    """Chord rules (`chord_progression*`) need a host analyser with the signature of the reference's piano_roll_to_chords
    (music21; not installable here).  --chord_backend module:function registers one (music_rules.register_chord_backend);
    --chord_backend native selects the device analyser instead (its own definition, docs/rounds/chords.md; --chord_profile picks its
    key profiles).
    Without one a config that asks for chord conditioning is an ERROR -- a run that silently lacks the requested rule would write
    tables that look like a fully conditioned one.  The explicit opt-in `--skip_chord_rules True` removes the chord entries from
    target_rules, from the SCG weights and from the cond_fn lists instead; what was removed is logged, recorded in
    run_metadata.json and marked in the output directory name (`_nochord`)."""
    from music_rule_guidance import music_rules
    del DROPPED_RULES[:]
    if getattr(args, "chord_backend", "") == "native":     # no colon: cannot collide with module:function
        music_rules.register_chord_backend("native", profile=getattr(args, "chord_profile", "krumhansl"))
        return config
    if getattr(args, "chord_backend", ""):
        import importlib
        mod, _, fn = args.chord_backend.partition(":")
        music_rules.register_chord_backend(getattr(importlib.import_module(mod), fn), workers=int(args.chord_workers))
        return config
    if music_rules._CHORD_BACKEND is not None:
        return config
    tr = vars(config.target_rules)
    cf = getattr(config.guidance, "cond_fn", None)
    wanted = [f"target_rules.{k}" for k in tr if "chord" in k]
    if cf is not None:
        wanted += [f"cond_fn.{r}" for r in cf.rule_names if "chord" in r]
    if not wanted:
        return config
    if not getattr(args, "skip_chord_rules", False):
        raise RuntimeError("this config conditions on chord rules (" + ", ".join(wanted) + ") but no chord analyser is registered: "
                           "pass --chord_backend module:function (signature of the reference's piano_roll_to_chords), or opt in to "
                           "running WITHOUT them with --skip_chord_rules True")
    dropped = []
    for k in [k for k in tr if "chord" in k]:
        tr.pop(k)
        dropped.append(f"target_rules.{k}")
    if getattr(config, "scg", None) is not None:
        for k in [k for k in vars(config.scg) if "chord" in k]:
            vars(config.scg).pop(k)
    if cf is not None and any("chord" in r for r in cf.rule_names):
        keep = [i for i, r in enumerate(cf.rule_names) if "chord" not in r]
        dropped += [f"cond_fn.{cf.rule_names[i]}" for i in range(len(cf.rule_names)) if i not in keep]
        for name in ("fns", "classifier_scales", "rule_names"):
            setattr(cf, name, [getattr(cf, name)[i] for i in keep])
        cc = getattr(cf, "classifiers", None)
        if cc is not None:
            for name in ("names", "paths", "num_classes"):
                if hasattr(cc, name):
                    v = getattr(cc, name)
                    setattr(cc, name, [v[i] for i in keep if i < len(v)])
        if not keep:
            config.guidance.cond_fn = None
            config.guidance.nn = False
    DROPPED_RULES.extend(dropped)
    logger.log("WARNING: --skip_chord_rules: running WITHOUT " + ", ".join(dropped))
    return config


def write_run_metadata(save_dir, args, extra=None):
    """run_metadata.json next to results.csv: what this run was NOT conditioned on / substituted (empty lists for a faithful run)."""
    import json
    meta = {"config_path": args.config_path, "dropped_rules": list(DROPPED_RULES), "synthetic_weights": bool(args.synthetic_weights),
            "targets_npz": getattr(args, "targets_npz", "") or None}
    from guided_diffusion.dit import long_backward
    meta["sampler"] = sampler_metadata(args)
    meta["chord_backend"] = getattr(args, "chord_backend", "") or None
    meta["chord_profile"] = getattr(args, "chord_profile", "krumhansl") if meta["chord_backend"] == "native" else None
    meta["note_stats"] = bool(getattr(args, "note_stats", False))   # notes.* columns in results.csv (docs/rounds/notes.md)
    meta["long_backward"] = bool(long_backward())     # RGM_LONG_BACKWARD / set_long_backward: guidance beyond 256 / 288 tokens was allowed
    meta["particles"] = particle_metadata(args)       # --particles: the particle loop in place of the SCG search (docs/rounds/particles.md)
    meta["midi_backend"] = getattr(args, "midi_backend", "host")    # who wrote the .midi files: the host loop or csrc/midi.hip (docs/rounds/midi.md)
    meta["wav"] = getattr(args, "wav", "off")         # .wav files beside the .midi: csrc/synth.hip's sine voice (docs/rounds/synth.md)
    meta["wav_fs"] = getattr(args, "wav_fs", 44100) if meta["wav"] != "off" else None
    meta.update(extra or {})
    with open(os.path.join(save_dir, "run_metadata.json"), "w") as f:
        json.dump(meta, f, indent=1)


NOTE_STATS_SCALARS = ("n_notes", "end_time", "total_used_pitch", "pitch_range", "avg_IOI", "mean_note_velocity", "mean_note_duration",
                      "note_density_mgeval")


def note_stats_columns(sample_u8, t0=None, t1=None):
    """--note_stats: mgeval's note statistics (docs/rounds/notes.md) of the uint8 rolls decode_sample_for_midi returns, (B, 128, T, 3) on
    the device, read there in place, as the saved MIDI files hold them (first-column onsets set) -> {"notes.<statistic>": one value per
    sample}: numbers for the scalar statistics, lists for the histogram (12) and the transition matrix (12 x 12)."""
    from music_rule_guidance import music_rules
    st = music_rules.note_stats(sample_u8 if t0 is None else sample_u8[:, :, t0:t1], first_column_onsets=True)
    cols = {"notes." + k: st[k].cpu().tolist() for k in NOTE_STATS_SCALARS}
    cols["notes.total_pitch_class_histogram"] = st["total_pitch_class_histogram"].cpu().tolist()
    cols["notes.pitch_class_transition_matrix"] = st["pitch_class_transition_matrix"].cpu().tolist()
    return cols


def device_midi_bytes(sample_u8, args):
    """--midi_backend device: the finished files of the uint8 rolls decode_sample_for_midi returns, formed on the device before the rolls
    are copied down (first-column onsets set, as save_piano_roll_midi sets them); None under the host backend."""
    if getattr(args, "midi_backend", "host") != "device":
        return None
    return midi_util.rolls_to_midi_bytes(sample_u8, fs=args.fs, first_column_onsets=True)


def device_wav_bytes(sample_u8, args):
    """--wav device: one finished .wav per uint8 roll, rendered and quantised on the device before the rolls are copied down; the audio
    holds the notes of the .midi written beside it (first-column onsets set); None under --wav off."""
    if getattr(args, "wav", "off") != "device":
        return None
    return midi_util.rolls_to_wav_bytes(sample_u8, fs=args.fs, audio_fs=args.wav_fs, first_column_onsets=True)


def summary_columns(all_results):
    """the columns summary.csv averages: the rule losses, and under --note_stats the scalar note statistics (NaN skipped)"""
    return [c for c in all_results.columns if ".loss" in c] + ["notes." + k for k in NOTE_STATS_SCALARS if "notes." + k in all_results.columns]


def choose_sampler(args, config):
    """The chain of this run, set in args.timestep_respacing before the diffusion is built.  --sampler config: what the YAML says (DDIM
    with eta = 1 on sampling.timestep_respacing when sampling.use_ddim, else the DDPM chain).  --sampler dpmpp: DPM-Solver++(2M) on
    --dpmpp_steps logSNR-uniform steps of the same schedule, whatever chain the YAML names."""
    if args.sampler not in ("config", "dpmpp"):
        raise ValueError(f"--sampler {args.sampler!r}: 'config' (the YAML's DDPM / DDIM chain) or 'dpmpp'")
    if config.sampling.use_ddim:
        args.timestep_respacing = config.sampling.timestep_respacing
    if args.sampler == "dpmpp":
        args.timestep_respacing = f"logsnr{int(args.dpmpp_steps)}"


def sampler_loop(args, config, diffusion):
    """The sampling loop choose_sampler picked, with the sampler's own arguments bound."""
    if args.sampler == "dpmpp":
        return partial(diffusion.dpmpp_sample_loop, order=int(args.dpmpp_order), eta=float(args.dpmpp_eta))
    return partial(diffusion.ddim_sample_loop, eta=1.) if config.sampling.use_ddim else diffusion.p_sample_loop


def sampler_metadata(args):
    name = getattr(args, "sampler", "config")
    if name != "dpmpp":
        return {"name": "config", "timestep_respacing": getattr(args, "timestep_respacing", "")}
    return {"name": "dpmpp", "timestep_respacing": args.timestep_respacing, "steps": int(args.dpmpp_steps),
            "order": int(args.dpmpp_order), "eta": float(args.dpmpp_eta)}


def particle_metadata(args):
    n = int(getattr(args, "particles", 0) or 0)
    if n < 2:
        return None
    return {"num_particles": n, "lambda": float(args.particle_lambda), "ess": float(args.particle_ess), "every": int(args.particle_every),
            "keep": args.particle_keep}


def particle_loop(args, config, diffusion):
    """--particles n >= 2: the config's target rules under diffusion.particle_sample_loop on the chain choose_sampler picked, forced
    stochastic (DDPM, DDIM at eta = 1, the SDE form of DPM-Solver++).  The rule weights are the YAML's `scg` block where present
    (scg.num_samples is ignored); every step is scored unless --particle_every says otherwise.  A gradient cond_fn passes through under
    the YAML's guidance schedule; DPS and segment-mode configs raise (GaussianDiffusion._particle_check).  Returns
    sample_fn(model, shape, **the sampling loops' keywords) -> the particle loop's result dict."""
    n = int(args.particles)
    if n < 2:
        raise ValueError(f"--particles {n}: 0 (off) or at least 2 particles per excerpt")
    pk = {k: v for k, v in vars(getattr(config, "scg", None) or argparse.Namespace()).items() if k != "num_samples"}
    pk.update({"lambda": float(args.particle_lambda), "ess": float(args.particle_ess), "every": int(args.particle_every)})
    name = "dpmpp" if args.sampler == "dpmpp" else ("ddim" if config.sampling.use_ddim else "ddpm")

    def sample_fn(model, shape, clip_denoised, model_kwargs, device, cond_fn, embed_model, scale_factor, guidance_kwargs, scg_kwargs,
                  t_end, record, progress):
        del scg_kwargs, record                       # the particle loop replaces the SCG search and keeps no per-step records
        return diffusion.particle_sample_loop(model, shape, n, sampler=name, particle_kwargs=pk, model_kwargs=model_kwargs,
                                              embed_model=embed_model, scale_factor=scale_factor, clip_denoised=clip_denoised,
                                              cond_fn=cond_fn, t_end=t_end, device=device, progress=progress,
                                              dpmpp_order=int(args.dpmpp_order), guidance_kwargs=guidance_kwargs)
    return sample_fn


def targets_from_npz(path, target_rules, batch_size, device):
    """`target_rules: Null` (reference :147-168: the targets are the rules of a dataset batch).  The dataset loader is out of scope;
    the batch itself is not: --targets_npz gives either `gt`, the ground-truth rolls ((B,3,128,T) float32 in [-1,1], what the
    reference's load_data yields) from which every rule is extracted with _extract_rule exactly like the reference does, or one
    array per rule ((B,K) or (K,)).  vertical_nd / horizontal_nd collapse into the fused note_density rule as in the reference."""
    names = list(target_rules)
    if "vertical_nd" in names:
        names = [k for k in names if k not in ("vertical_nd", "horizontal_nd")] + ["note_density"]
    z = np.load(path)
    out = {}
    if "gt" in z.files:
        gt = th.from_numpy(np.ascontiguousarray(z["gt"], dtype=np.float32)).to(device)
        if gt.shape[0] < batch_size:
            raise ValueError(f"{path}: gt holds {gt.shape[0]} rolls, batch_size is {batch_size}")
        gt = gt[:batch_size].contiguous()
        with th.no_grad():
            for k in names:
                out[k] = _extract_rule(k, gt)
        return out
    for k in names:
        if k not in z.files:
            raise KeyError(f"{path}: no array for rule '{k}' (has {z.files}); give `gt` or one array per rule")
        v = th.from_numpy(np.ascontiguousarray(z[k])).to(device)
        v = v.float() if v.is_floating_point() else v
        if v.dim() == 1:
            v = v.repeat(batch_size, 1)
        if v.shape[0] < batch_size:
            raise ValueError(f"{path}: '{k}' holds {v.shape[0]} rows, batch_size is {batch_size}")
        out[k] = v[:batch_size].contiguous()
    return out


def check_target_lengths(rules, frames, device):
    """Every length-dependent rule target must have the length that rule has on the rolls this run makes (`frames` time steps,
    8 per latent row: --image_size H 16 gives 8H).  note_density has 2 values per 128 frames, so the shipped YAML lists (made for
    1024 frames) do not fit a longer excerpt: refused here with both lengths named, not deep inside the loss."""
    probe = th.full((1, 3, 128, frames), -1.0, device=device)
    for name, target in rules.items():
        if "chord" in name or name not in midi_util.FUNC_DICT:
            continue
        with th.no_grad():
            n = int(midi_util.FUNC_DICT[name](probe).shape[-1])
        k = int(target.shape[-1])
        if k != n:
            raise ValueError(f"rule '{name}': the target has {k} values, which fits a roll of {frames * k // max(n, 1)} frames, but this "
                             f"run makes rolls of {frames} frames (--image_size {frames // 8} 16), where '{name}' has {n} values")


def output_dir_for(config_path, class_label):
    """cond_demo/<config path below cond_table/ or cond_demo/>_cls_<label>   (reference :42-46)."""
    root = "cond_demo/"
    key = "cond_table/" if "cond_table/" in config_path else root
    return root + os.path.splitext(config_path.split(key)[-1])[0] + f"_cls_{class_label}"


def build_target_rules(target_rules, batch_size, device):
    """YAML target lists -> {rule: (B,K) tensor}.  vertical_nd + horizontal_nd fuse into one note_density
    target [vertical..., horizontal/scale...] (scale 5, or N for the *_hr_N variants); pitch_hist is
    normalised to sum 1 (reference :170-193)."""
    rules = dict(target_rules)
    for key in list(rules):
        if "vertical_nd" in key:
            if "_hr_" in key:
                tag = key.split("_hr_")[-1]
                scale, hkey, out = int(tag), f"horizontal_nd_hr_{tag}", f"note_density_hr_{tag}"
            else:
                scale, hkey, out = 5, "horizontal_nd", "note_density"
            rules[out] = list(rules[key]) + [v / scale for v in rules[hkey]]
            rules.pop(key)
            rules.pop(hkey)
            break
    out = {}
    for key, val in rules.items():
        v = th.tensor(val, device=device)
        if key == "pitch_hist":
            v = v / (th.sum(v) + 1e-12)
        out[key] = v.repeat(batch_size, 1)
    return out


def build_pipeline(args, config, device):
    """eps-network, diffusion, VAE, guidance cond_fn and the (possibly DiffCollage-wrapped) model_fn, as both CLIs
    (sample_rule.py :52-137, edit.py :55-138 of the reference) set them up.  Returns a SimpleNamespace."""
    from types import SimpleNamespace
    logger.log("creating model and diffusion...")
    model = DiT_models[args.model](input_size=args.image_size, in_channels=args.in_channels,
                                   num_classes=args.num_classes, learn_sigma=args.learn_sigma)
    diffusion = create_diffusion(**args_to_dict(args, ["learn_sigma", "diffusion_steps", "noise_schedule", "timestep_respacing",
                                                       "use_kl", "predict_xstart", "rescale_timesteps", "rescale_learned_sigmas"]))
    if args.synthetic_weights:
        from rgm import synth
        arch = dict(depth=model.depth, hidden=model.hidden_size, heads=model.num_heads, patch=model.patch_size,
                    in_ch=args.in_channels, out_ch=model.out_channels,
                    num_classes=model._n_embed, class_dropout=False)
        model.load_state_dict(synth.dit_state_dict(1, final_std=0.3 / model.hidden_size ** 0.5, device=device, **arch))
    else:
        model.load_state_dict(dist_util.load_state_dict(args.model_path, map_location="cpu"), strict=False)
    model.to(device)
    if args.use_fp16:
        raise NotImplementedError("the reference's DiTRotary has no convert_to_fp16 either; sampling is fp32")
    model.eval()

    embed_model = None
    if args.vae is not None:
        embed_model = load_model(args.vae, None if args.synthetic_weights else args.vae_path)
        if args.synthetic_weights:
            from rgm import synth
            embed_model.load_state_dict(synth.vae_state_dict(2, device=device, encoder=True))
        embed_model.to(device)
        embed_model.eval()

    cond_fn_config = config.guidance.cond_fn
    classifiers = []
    if config.guidance.nn:
        logger.log("loading classifier...")
        cc = cond_fn_config.classifiers
        # the reference loads one classifier per entry of `names` (:88-104; cond_demo/demo3.yml lists three cond_fns but two
        # names, so two run); its pixel-space ablation configs carry no names at all: inferred from the cond_fn here
        names = getattr(cc, "names", None) or ["DiTRotary-S/8-chord-cls" if "chord" in f else "DiTRotary-S/8-cls" for f in cond_fn_config.fns]
        for i, name in enumerate(names):
            clf = DiT_models[name](input_size=args.image_size, in_channels=args.in_channels, num_classes=cc.num_classes[i])
            if args.synthetic_weights:
                from rgm import synth
                arch = dict(depth=clf.depth, hidden=clf.hidden_size, heads=clf.num_heads, patch=clf.patch_size,
                            in_ch=args.in_channels, classifier=True, cls_classes=cc.num_classes[i], chord=clf.chord)
                clf.load_state_dict(synth.dit_state_dict(3 + i, device=device, **arch))
            else:
                clf.load_state_dict(dist_util.load_state_dict(cc.paths[i], map_location="cpu"))
            clf.to(device)
            clf.eval()
            classifiers.append(clf)

    if cond_fn_config is None:
        cond_fn_used = None
    elif config.guidance.nn:
        cond_fn_used = partial(composite_nn_zt, fns=cond_fn_config.fns, classifier_scales=cond_fn_config.classifier_scales,
                               classifiers=classifiers, rule_names=cond_fn_config.rule_names)
    else:
        cond_fn_used = partial(composite_rule, fns=cond_fn_config.fns, classifier_scales=cond_fn_config.classifier_scales,
                               rule_names=cond_fn_config.rule_names)

    if config.sampling.diff_collage:
        def eps_fn(x, t, y=None):          # the backbone takes (4, time, pitch)
            return model(x.permute(0, 1, 3, 2).contiguous(), t, y=y).permute(0, 1, 3, 2)
        img_shape = (args.in_channels, args.image_size[1], args.image_size[0])            # 4 x 16 x 128
        if config.dc.type == "circle":       # the circle needs one more window than the line
            worker = dc.CondIndCircle(img_shape, eps_fn, config.dc.num_img + 1, overlap_size=config.dc.overlap_size)
        else:
            worker = dc.CondIndSimple(img_shape, eps_fn, config.dc.num_img, overlap_size=config.dc.overlap_size)
        gen_shape = (args.batch_size, worker.shape[0], worker.shape[2], worker.shape[1])
        model_fn_used = partial(dc_model_fn, model=worker.eps_scalar_t_fn, num_classes=args.num_classes,
                                class_cond=args.class_cond, cfg=args.cfg, w=args.w)
    else:
        gen_shape = (args.batch_size, args.in_channels, args.image_size[0], args.image_size[1])
        model_fn_used = partial(model_fn, model=model, num_classes=args.num_classes, class_cond=args.class_cond,
                                cfg=args.cfg, w=args.w)

    return SimpleNamespace(model=model, diffusion=diffusion, embed_model=embed_model, cond_fn=cond_fn_used,
                           model_fn=model_fn_used, gen_shape=gen_shape, classifiers=classifiers)


def main(argv=None):
    args = add_wav_arguments(add_midi_arguments(add_particle_arguments(add_note_stats_arguments(add_sampler_arguments(create_argparser()))))).parse_args(argv)
    args.dir = output_dir_for(args.config_path, args.class_label)
    from rgm import native as _native
    _native.set_gemm_precision(args.gemm_precision)      # "bf16x3_presplit" / "bf16x3" (fast, fp32-grade) or "fp32" (exact fp32 MFMA)
    comm = dist_util.setup_dist(port=args.port)
    config = setup_chord_backend(args, midi_util.load_config(args.config_path))
    if DROPPED_RULES:
        args.dir += "_nochord"
    logger.configure(args=args, comm=comm)
    choose_sampler(args, config)
    device = dist_util.dev()
    rank0 = int(os.environ.get("RANK", "0")) == 0

    P = build_pipeline(args, config, device)
    diffusion, embed_model, cond_fn_used, model_fn_used, gen_shape = P.diffusion, P.embed_model, P.cond_fn, P.model_fn, P.gen_shape
    diffusion.noise_fn = NOISE_FN

    target_rules = vars(config.target_rules)
    if any(v is None for v in list(target_rules.values())[:1]):
        if not args.targets_npz:
            raise NotImplementedError("target rules 'Null' are the rules of a dataset batch in the reference (:147-168); the dataset "
                                      "loader is out of scope -- pass that batch with --targets_npz (`gt` rolls or one array per "
                                      "rule), or give the targets in the YAML")
        model_kwargs = {"rule": targets_from_npz(args.targets_npz, target_rules, args.batch_size, device)}
    else:
        model_kwargs = {"rule": build_target_rules(target_rules, args.batch_size, device)}
    check_target_lengths(model_kwargs["rule"], 8 * gen_shape[2], device)
    classes = None
    if args.class_cond:
        classes = th.ones(size=(args.batch_size,), device=device, dtype=th.int) * args.class_label
        model_kwargs["y"] = classes

    save_dir = logger.get_dir()
    os.makedirs(os.path.expanduser(save_dir), exist_ok=True)
    if args.save_files and rank0:
        write_run_metadata(save_dir, args)
    particles = int(args.particles) != 0
    sample_fn = particle_loop(args, config, diffusion) if particles else sampler_loop(args, config, diffusion)
    use_scg = bool(getattr(config.guidance, "scg", getattr(config.guidance, "beam", False)))

    logger.log("sampling...")
    count_samples = 0
    all_results = pd.DataFrame()
    while count_samples < args.num_samples:
        sample = sample_fn(
            model_fn_used, gen_shape, clip_denoised=args.clip_denoised, model_kwargs=model_kwargs, device=device,
            cond_fn=cond_fn_used, embed_model=embed_model if config.guidance.vae else None, scale_factor=args.scale_factor,
            guidance_kwargs=config.guidance, scg_kwargs=vars(config.scg) if use_scg else None,
            t_end=config.sampling.t_end, record=args.record, progress=args.progress)
        rules_of, classes_of, particle_cols = model_kwargs["rule"], classes, {}
        if particles:                                      # 'best': B rolls, results.csv as ever; 'all': n B rolls, row k B + b = particle k of excerpt b
            res = sample
            sample = res["best"] if args.particle_keep == "best" else res["sample"]
            if args.particle_keep == "all":
                n = int(args.particles)
                rules_of = {k: v.repeat(n, 1) for k, v in model_kwargs["rule"].items()}
                classes_of = classes.repeat(n) if classes is not None else None
                particle_cols = {"particle": th.arange(n).repeat_interleave(args.batch_size).tolist(),
                                 "log_weight": res["log_weights"].reshape(-1).cpu().tolist()}
        if KEEP_FLOAT_ROLLS is not None:        # parity tests: the float roll explains every uint8 difference (boundary adjacency)
            from guided_diffusion.gaussian_diffusion import _decode
            with _native.gemm_precision_scope("fp32" if midi_util.FINAL_DECODE_EXACT else None):   # the final decode's own arithmetic
                KEEP_FLOAT_ROLLS.append(_decode(sample, embed_model, scale_factor=args.scale_factor).float().cpu().numpy())
        sample = midi_util.decode_sample_for_midi(sample, embed_model=embed_model, scale_factor=args.scale_factor, threshold=-0.95)
        note_cols = note_stats_columns(sample) if args.note_stats else {}                  # on the device, before the roll leaves it
        midi_bytes = device_midi_bytes(sample, args) if args.save_files and rank0 else None
        wav_files = device_wav_bytes(sample, args) if args.save_files and rank0 else None
        arr = sample.cpu().numpy().transpose(0, 3, 1, 2)                                   # (B, 3, 128, T) uint8
        if args.save_files and rank0:
            midi_util.save_piano_roll_midi(arr, save_dir, args.fs, y=classes_of.cpu().numpy() if classes_of is not None else None,
                                           save_ind=count_samples * (arr.shape[0] // args.batch_size), midi_bytes=midi_bytes,
                                           wav_bytes=wav_files)
        generated = th.from_numpy(arr.astype(np.float32)) / 63.5 - 1
        results = midi_util.eval_rule_loss(generated, rules_of)
        for name, col in list(note_cols.items()) + list(particle_cols.items()):
            results[name] = col
        all_results = pd.concat([all_results, results], ignore_index=True)
        if args.save_files and rank0:
            all_results.to_csv(os.path.join(save_dir, "results.csv"), index=False)
        count_samples += args.batch_size

    if args.save_files and rank0:
        loss_cols = summary_columns(all_results)
        stats = pd.DataFrame([{"Attr": c, "Mean": all_results[c].mean(), "Std": all_results[c].std()} for c in loss_cols],
                             columns=["Attr", "Mean", "Std"])
        stats.to_csv(os.path.join(save_dir, "summary.csv"))
        print(stats)
    if args.record and rank0:
        import pickle
        for name in ("log_probs", "loss_std", "loss_range", "each_loss"):
            with open(os.path.join(save_dir, name + ".pkl"), "wb") as f:
                pickle.dump(dict(getattr(diffusion, name)) if name == "each_loss" else getattr(diffusion, name), f)
    logger.log("sampling complete")
    return all_results


def create_argparser():
    defaults = dict(
        project="music-sampling", dir="", data_dir="", config_path="", model="DiTRotary_XL_8", model_path="",
        vae="kl/f8-all-onset", vae_path="taming-transformers/checkpoints/all_onset/epoch_14.ckpt",
        clip_denoised=False, num_samples=128, batch_size=16, scale_factor=1., fs=100, num_classes=0, class_label=1,
        cfg=False, w=4., classifier_scale=1.0, record=False, save_files=True, training=False, deterministic=False,
        port=None,
        # additions of this implementation
        synthetic_weights=False, progress=True, gemm_precision="bf16x3_presplit", chord_backend="", chord_workers=4,
        skip_chord_rules=False, targets_npz="",
    )
    defaults.update(model_and_diffusion_defaults())
    parser = argparse.ArgumentParser()
    add_dict_to_argparser(parser, defaults)
    return parser


def add_sampler_arguments(parser):
    """--sampler and the DPM-Solver++ options (and --chord_profile of the native chord analyser): the groups sample_rule.py and edit.py
    share, with the choices and help texts that the defaults dictionary of create_argparser (the reference's flags) cannot carry."""
    g = parser.add_argument_group("sampler")
    g.add_argument("--sampler", default="config", choices=["config", "dpmpp"],
                   help="'config': the YAML's chain (DDPM, or DDIM with eta = 1 on sampling.timestep_respacing); 'dpmpp': DPM-Solver++(2M) "
                        "on --dpmpp_steps logSNR-uniform steps of the same schedule")
    g.add_argument("--dpmpp_steps", type=int, default=20, help="targets of the logSNR-uniform chain (timestep_respacing 'logsnrN')")
    g.add_argument("--dpmpp_order", type=int, default=2, choices=[1, 2], help="2: the multistep solver; 1: first order throughout")
    g.add_argument("--dpmpp_eta", type=float, default=1.0, choices=[0.0, 1.0],
                   help="1: the SDE form (stochastic; what SCG needs to have candidates); 0: the probability-flow ODE")
    g = parser.add_argument_group("chord analyser")
    g.add_argument("--chord_profile", default="krumhansl", choices=["krumhansl", "aarden"],
                   help="key profiles of --chord_backend native (Krumhansl-Kessler or Aarden-Essen)")
    return parser


def add_note_stats_arguments(parser):
    """--note_stats: the opt-in notes.* report columns of sample_rule.py and edit.py (kept out of create_argparser's defaults, which
    mirror the reference's flags)."""
    g = parser.add_argument_group("note statistics")
    g.add_argument("--note_stats", default=False, type=str2bool,
                   help="True: mgeval's note statistics of every saved roll (used pitches, pitch range, average IOI, pitch-class histogram, "
                        "mean velocity / duration, notes per second, transition matrix) as notes.* columns of results.csv, their means in "
                        "summary.csv; computed on the device (docs/rounds/notes.md)")
    return parser


def add_midi_arguments(parser):
    """--midi_backend: who turns the final rolls into .midi files, shared by sample_rule.py, edit.py and cfg_sample.py (kept out of
    create_argparser's defaults like the groups above; docs/rounds/midi.md)."""
    g = parser.add_argument_group("MIDI writer")
    g.add_argument("--midi_backend", default="host", choices=list(midi_util.MIDI_BACKENDS),
                   help="'host': piano_roll_to_pretty_midi and SimpleMIDI.write, one sample after the other; 'device': the same bytes formed by "
                        "csrc/midi.hip for the whole batch while the rolls are still on the device (fs <= 220)")
    return parser


def add_wav_arguments(parser):
    """--wav and --wav_fs: audio beside the .midi files, shared by sample_rule.py and edit.py (cfg_sample.py adds the same two flags; kept
    out of create_argparser's defaults and in a group of their own like --midi_backend; docs/rounds/synth.md)."""
    g = parser.add_argument_group("audio")
    g.add_argument("--wav", default="off", choices=list(midi_util.WAV_BACKENDS),
                   help="'device': a sample_<i>.wav beside every .midi, the roll's notes as sines rendered by csrc/synth.hip (mono, 16 bit; "
                        "docs/rounds/synth.md); 'off': none")
    g.add_argument("--wav_fs", type=int, default=44100, help="audio samples per second of the .wav files")
    return parser


def add_midi_reader_arguments(parser):
    """--midi_reader: who turns a MIDI source into a piano roll, for edit.py and midi_to_rolls.py (kept out of create_argparser's
    defaults and out of add_midi_arguments; docs/rounds/midi_read.md)."""
    g = parser.add_argument_group("MIDI reader")
    g.add_argument("--midi_reader", default="host", choices=list(midi_util.MIDI_READERS),
                   help="'host': SimpleMIDI and midi_to_full_piano_roll, one byte, event and note after the other; 'device': the same roll "
                        "built by csrc/midi_read.hip (a reader registered with register_midi_reader wins either way)")
    return parser


def add_particle_arguments(parser):
    """--particles and its options: particle rule guidance (sequential Monte Carlo) in place of the SCG search, kept out of
    create_argparser's defaults like the two groups above (docs/rounds/particles.md)."""
    g = parser.add_argument_group("particle rule guidance")
    g.add_argument("--particles", type=int, default=0,
                   help="n >= 2: run the config's target rules under the particle loop with n particles per excerpt (rule weights from the "
                        "YAML's scg block, scg.num_samples ignored; the sampler forced stochastic); 0: off")
    g.add_argument("--particle_lambda", type=float, default=1.0, help="the tilt: the particles target p(x0) exp(lambda r(x0))")
    g.add_argument("--particle_ess", type=float, default=0.5,
                   help="resample a group where its effective sample size falls below this fraction of n (<= 0 never, > 1 always)")
    g.add_argument("--particle_every", type=int, default=1, help="score and resample on every k-th step")
    g.add_argument("--particle_keep", default="best", choices=["best", "all"],
                   help="'best': one roll per excerpt, the particle of the highest final reward; 'all': every particle's roll, with "
                        "`particle` and `log_weight` columns in results.csv")
    return parser


if __name__ == "__main__":
    main()
