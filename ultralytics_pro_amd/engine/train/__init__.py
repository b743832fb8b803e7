"""The training step by concern (the map is in `engine/trainer.py`, which re-exports the public names).  Nothing is imported here:
`targets` stays importable without the library."""
