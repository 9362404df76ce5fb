"""The reference's import path music_evaluation/mgeval/utils.py, on device tensors."""
