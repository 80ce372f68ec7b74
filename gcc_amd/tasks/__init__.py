"""Downstream tasks on the embeddings ``generate.py`` writes (gcc/tasks of the reference)."""
