"""Objective evaluation of sets of samples on the device: mgeval's set-level distances, KL divergence and overlap area (set_eval.py,
mgeval/utils.py; docs/rounds/sets.md).  The per-sample statistics are music_rule_guidance.music_rules.note_stats."""
