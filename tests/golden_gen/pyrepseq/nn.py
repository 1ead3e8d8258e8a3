"""Stand-in for pyrepseq.nn.symdel as the reference's make_merge_groups calls it (collapse.py:735-740): every ordered pair
(i, j), i != j, of strings within Levenshtein distance max_edits, as a scipy coo_matrix of ones.  Brute force with two exact
prefilters (length difference and composition L1 distance, both lower bounds of the distance), decided by the polyleven
stand-in of oracle/refshim.  Dev-machine fixture generation only."""
import numpy as np
import polyleven
from scipy import sparse


def symdel(seqs, max_edits=1, progress=False, output_type="coo_matrix", **_):
    seqs = list(seqs)
    n = len(seqs)
    alphabet = sorted(set("".join(seqs)))
    comp = np.array([[s.count(c) for c in alphabet] for s in seqs], dtype=np.int32).reshape(n, len(alphabet))
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    rows, cols = [], []
    for i in range(n):
        j = np.arange(i + 1, n)
        ok = (np.abs(lens[j] - lens[i]) <= max_edits) & (np.abs(comp[j] - comp[i]).sum(axis=1) <= 2 * max_edits)
        for jj in j[ok].tolist():
            if polyleven.levenshtein(seqs[i], seqs[jj]) <= max_edits:
                rows += [i, jj]
                cols += [jj, i]
    return sparse.coo_matrix((np.ones(len(rows), dtype=np.int64), (rows, cols)), shape=(n, n))
