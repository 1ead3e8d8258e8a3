"""Stand-in package for pyrepseq, for gen_collapse_cluster.py only (the wheel is not installable offline)."""
