"""Gene-family tag sets and the reads that contest them (TEST INFRASTRUCTURE).

decombinator_amd.synth builds tag sets whose tags are pairwise three or more
substitutions apart, so a window of a read is within Hamming 1 of one tag at
most and the reference's candidate order (decombine.py:292-394, :420-531: half
tag hits in findall order, the genes sharing the half in index order, the first
one that passes Hamming <= 1 and whose walk succeeds) decides nothing.  Real V
and J families are near-identical paralogues.  This module builds such sets:

* make_family_tagset  - equal-length tags in families that share a half and lie
                        1 or 2 substitutions apart in the other one
* contested_reads     - rearrangements whose tag is overwritten by a "midpoint",
                        a string within Hamming 1 of two family members
* decoy_ladder        - rearrangements behind (V) or in front of (J) a ladder of
                        k bare half tags, on both sides of the kernels' list limits
* is_contested        - how many tags lie within Hamming 1 of the windows a
                        record settled on

oracle/gen_golden.py and the tests import it; nothing under decombinator_amd/ does.
"""
from __future__ import annotations

import functools

import numpy as np

from decombinator_amd import synth
from oracle import casegen

LADDER_KS = (3, 4, 5, 7, 8, 9, 10)


def hamming(a: str, b: str) -> int:
    return sum(x != y for x, y in zip(a, b)) if len(a) == len(b) else max(len(a), len(b))


def pairs_at(tags, d: int):
    """[(a, b)], a < b, of the tags exactly d substitutions apart."""
    return [(a, b) for a in range(len(tags)) for b in range(a + 1, len(tags)) if hamming(tags[a], tags[b]) == d]


def _set_base(s: str, pos: int, base: str) -> str:
    return s[:pos] + base + s[pos + 1:]


def _other_base(rng, s: str, pos: int, avoid: str = "") -> str:
    return str(rng.choice([b for b in "ACGT" if b != s[pos] and b not in avoid]))


def midpoints(a: str, b: str):
    """The two strings one substitution from each of a and b (Hamming(a, b) == 2)."""
    p, q = [i for i in range(len(a)) if a[i] != b[i]]
    return [_set_base(a, p, b[p]), _set_base(a, q, b[q])]


# --------------------------------------------------------------------------------------------------------------
# the tag set
# --------------------------------------------------------------------------------------------------------------

def _family_tags(rng, n: int, tag_len: int, split: int, n_families: int, sizes):
    """(tags, families) before the shuffle: families as lists of indices."""
    while True:
        tags, fams = [], []
        for f in range(n_families):
            other = list(range(split, tag_len)) if f % 2 == 0 else list(range(0, split))
            size = int(rng.integers(sizes[0], sizes[1] + 1))
            while True:
                members = [casegen.rand_seq(rng, tag_len)]
                while len(members) < size:
                    m = members[int(rng.integers(0, len(members)))]
                    for p in rng.choice(other, size=int(rng.integers(1, 3)), replace=False):
                        m = _set_base(m, int(p), _other_base(rng, m, int(p)))
                    if m not in members:
                        members.append(m)
                if all(hamming(m, t) >= 3 for m in members for t in tags):
                    break
            fams.append(list(range(len(tags), len(tags) + size)))
            tags.extend(members)
        assert len(tags) < n, "the families leave no room for a tag outside them"
        while len(tags) < n:
            t = casegen.rand_seq(rng, tag_len)
            if all(hamming(t, u) >= 3 for u in tags):
                tags.append(t)
        if len(pairs_at(tags, 1)) >= 2 and len(pairs_at(tags, 2)) >= 4:
            return tags, fams


def _place_decoy(rng, region: str, tagoff: int, half: str) -> str:
    d = int(rng.integers(max(12, len(half) + 1), 51))
    return region[:tagoff - d] + half + region[tagoff - d + len(half):]


def make_family_tagset(seed: int, tags: str = "original", chain: str = "b", n_v: int = 40, n_j: int = 12,
                       tag_len: int = 20, v_families: int = 5, j_families: int = 2, related_regions: bool = True,
                       decoys: bool = True, species: str = "human") -> synth.TagSet:
    """A seeded tag set of gene families.  Even families share half 1, odd ones half 2 (at the set's own split);
    every member lies 1 or 2 substitutions from an earlier one in the other half; tags outside families are 3 or
    more from everything.  ts.v_families / ts.j_families list the members' gene indices (after the shuffle)."""
    rng = np.random.default_rng(seed)
    ts = synth.TagSet(species=species, tags=tags, chain=chain)
    v_split, j_split = ts.half_splits
    for gene, n, split, n_fam, sizes in (("v", n_v, v_split, v_families, (3, 6)), ("j", n_j, j_split, j_families, (3, 4))):
        tg, fams = _family_tags(rng, n, tag_len, split, n_fam, sizes)
        while True:                                                      # shuffled: no family on consecutive indices
            order = [int(x) for x in rng.permutation(n)]                 # order[new index] = old index
            new_of = {old: new for new, old in enumerate(order)}
            shuffled = [sorted(new_of[m] for m in fam) for fam in fams]
            if all(fam != list(range(fam[0], fam[0] + len(fam))) for fam in shuffled):
                break
        tg, fams = [tg[old] for old in order], shuffled
        fam_of = {m: f for f, fam in enumerate(fams) for m in fam}
        setattr(ts, f"{gene}_tags", tg)
        setattr(ts, f"{gene}_families", fams)
        # every family sits on one ancestor: its members' regions are that ancestor with a few substitutions
        anc = [(casegen.rand_seq(rng, 340), casegen.rand_seq(rng, 60)) for _ in fams]
        for i, t in enumerate(tg):
            if gene == "v":
                jump = int(synth.V_JUMPS[rng.integers(0, len(synth.V_JUMPS))])
                n_left, n_right = int(rng.integers(280, 341)) - jump, jump - tag_len
            else:
                jump = 20
                n_left, n_right = jump, max(0, int(rng.integers(47, 67)) - jump - tag_len)
            if related_regions and i in fam_of:
                a_left, a_right = anc[fam_of[i]]
                left = synth._mutate(rng, a_left[len(a_left) - n_left:], int(rng.integers(1, 5)))
                right = a_right[:n_right]
                if n_right:
                    right = synth._mutate(rng, right, int(rng.integers(0, min(3, n_right + 1))))
            else:
                left, right = casegen.rand_seq(rng, n_left), casegen.rand_seq(rng, n_right)
            reg = left + t + right
            if gene == "v" and decoys and rng.random() < 2 / 3:
                g = i if rng.random() < 0.5 else int(rng.integers(0, n))
                half = tg[g][:split] if rng.random() < 0.5 else tg[g][split:]
                reg = _place_decoy(rng, reg, n_left, half)
            getattr(ts, f"{gene}_jumps").append(jump)
            getattr(ts, f"{gene}_names").append(f"TR{chain.upper()}{gene.upper()}{i + 1}")
            getattr(ts, f"{gene}_regions").append(reg)
    check_family_tagset(ts)
    return ts


def check_family_tagset(ts) -> dict:
    """The generator's guarantees, asserted; returns the pair counts."""
    out = {}
    for gene, split in zip("vj", ts.half_splits):
        tg, fams = getattr(ts, f"{gene}_tags"), getattr(ts, f"{gene}_families")
        jumps, regions = getattr(ts, f"{gene}_jumps"), getattr(ts, f"{gene}_regions")
        assert len({len(t) for t in tg}) == 1 and len(set(tg)) == len(tg)
        in_fam = {m for fam in fams for m in fam}
        d1, d2 = pairs_at(tg, 1), pairs_at(tg, 2)
        assert len(d1) >= 2 and len(d2) >= 4, (gene, len(d1), len(d2))
        for f, fam in enumerate(fams):
            assert 3 <= len(fam) <= 6
            half = (lambda t: t[:split]) if f % 2 == 0 else (lambda t: t[split:])
            assert len({half(tg[m]) for m in fam}) == 1
            assert fam != list(range(fam[0], fam[0] + len(fam))), "a family on consecutive gene indices"
        for a in range(len(tg)):
            for b in range(a + 1, len(tg)):
                if hamming(tg[a], tg[b]) < 3:
                    assert a in in_fam and b in in_fam and any(a in fam and b in fam for fam in fams)
        for i, (t, jump, reg) in enumerate(zip(tg, jumps, regions)):
            off = len(reg) - jump if gene == "v" else jump
            assert reg[off:off + len(t)] == t, (gene, i)
            for u in tg:
                k = reg.find(u)
                assert k < 0 or (k == off and u == t and reg.find(u, k + 1) < 0), (gene, i, "a full tag beside the gene's own")
        out[gene] = {"d1": len(d1), "d2": len(d2), "families": [len(f) for f in fams]}
    return out


def tagset_from_dict(d: dict) -> synth.TagSet:
    """A fixture's "tagset" back as a TagSet (without the family lists: they follow from the tags)."""
    return synth.TagSet(species=d["species"], tags=d["tags"], chain=d["chain"], v_tags=d["v_tags"], v_jumps=d["v_jumps"],
                        v_names=d["v_names"], v_regions=d["v_regions"], j_tags=d["j_tags"], j_jumps=d["j_jumps"],
                        j_names=d["j_names"], j_regions=d["j_regions"])


# --------------------------------------------------------------------------------------------------------------
# contested reads
# --------------------------------------------------------------------------------------------------------------

MARKS_DTYPE = np.dtype([("src_v", "<i4"), ("src_j", "<i4"), ("contested_v", "?"), ("contested_j", "?"),
                        ("k_v", "<i4"), ("k_j", "<i4")])


def _partners(tags, d: int = 2):
    out = {}
    for a, b in pairs_at(tags, d):
        out.setdefault(a, []).append(b)
        out.setdefault(b, []).append(a)
    return out


def _midpoint_choices(tags, partners):
    """gene -> the midpoints between its tag and a partner's that are no tag themselves."""
    tagset = set(tags)
    return {g: [m for u in us for m in midpoints(tags[g], tags[u]) if m not in tagset] for g, us in partners.items()}


def contested_reads(ts, rng, n: int, p_v: float = 0.5, p_j: float = 1 / 3, p_sub: float = 0.2, p_cut: float = 0.1,
                    lengths=(150, 151, 101, 75), length_p=(0.45, 0.35, 0.1, 0.1)):
    """n sense-frame reads (casegen.rearranged) and their marks: source genes, contested_v / contested_j.
    About p_v of them carry a midpoint of the source V gene's family over the V tag, about p_j one over the J tag
    (where the tag lies inside the read), p_sub get 1-3 further substitutions anywhere, p_cut lose up to 30 nt at
    either end.  (The per-read draws are made up front, n at a time: a generator call per read and draw costs more
    than building the read.)"""
    mv, mj = _midpoint_choices(ts.v_tags, _partners(ts.v_tags)), _midpoint_choices(ts.j_tags, _partners(ts.j_tags))
    elig_v, elig_j = sorted(g for g in mv if mv[g]), sorted(g for g in mj if mj[g])
    nv, nj = len(ts.v_tags), len(ts.j_tags)
    u = rng.random((n, 12))
    want_v, want_j = u[:, 0] < p_v, u[:, 1] < p_j
    v = np.where(want_v, np.array(elig_v)[(u[:, 2] * len(elig_v)).astype(int)], (u[:, 2] * nv).astype(int)).tolist()
    j = np.where(want_j, np.array(elig_j)[(u[:, 3] * len(elig_j)).astype(int)], (u[:, 3] * nj).astype(int)).tolist()
    length = np.array(lengths)[np.searchsorted(np.cumsum(length_p), u[:, 4], side="right").clip(0, len(lengths) - 1)].tolist()
    vdel, jdel = rng.integers(0, 11, size=n).tolist(), rng.integers(0, 13, size=n).tolist()
    ins, vts = rng.integers(0, 26, size=n).tolist(), rng.integers(20, 61, size=n).tolist()
    n_sub = np.where(u[:, 5] < p_sub, rng.integers(1, 4, size=n), 0).tolist()
    cut = np.where(u[:, 6] < p_cut, rng.integers(1, 31, size=n), 0).tolist()
    want_v, want_j, u = want_v.tolist(), want_j.tolist(), u.tolist()
    reads, marks = [], np.zeros(n, dtype=MARKS_DTYPE)
    for r in range(n):
        read, info = casegen.rearranged(ts, rng, v[r], j[r], vdel[r], jdel[r], ins[r], vts[r], length[r])
        did_v = did_j = False
        if want_v[r]:
            ms, p = mv[v[r]], info["v_tag_pos"]
            m = ms[int(u[r][7] * len(ms))]
            if p + len(m) <= len(read):
                read, did_v = read[:p] + m + read[p + len(m):], True
        if want_j[r]:
            ms, p = mj[j[r]], info["j_tag_pos"]
            m = ms[int(u[r][8] * len(ms))]
            if p + len(m) <= len(read):
                read, did_j = read[:p] + m + read[p + len(m):], True
        for k in range(n_sub[r]):
            read = casegen.substitute(rng, read, int(u[r][9 + k] * len(read)))
        if cut[r]:
            read = read[cut[r]:] if u[r][6] < p_cut / 2 else read[:len(read) - cut[r]]
        reads.append(read)
        marks[r] = (v[r], j[r], did_v, did_j, 0, 0)
    return reads, marks


# --------------------------------------------------------------------------------------------------------------
# the decoy ladder
# --------------------------------------------------------------------------------------------------------------

def _halves(tags, split: int, kind: int):
    return [t[:split] if kind == 1 else t[split:] for t in tags]


@functools.lru_cache(maxsize=64)
def _half_pool(tags: tuple, split: int, kind: int):
    halves = _halves(tags, split, kind)
    return halves, sorted(set(halves))


def _ladder_halves(rng, tags, split: int, kind: int, own: int, k: int):
    """k half tags (kind 1 or 2) of other genes than `own`, neighbours different, all different while the set lasts."""
    halves, distinct = _half_pool(tuple(tags), split, kind)
    pool = [h for h in distinct if h != halves[own]]
    out = []
    while len(out) < k:
        for i in rng.permutation(len(pool)).tolist():
            if len(out) < k and (not out or out[-1] != pool[i]):
                out.append(pool[i])
    return out


def _sub_in_half(rng, tag: str, split: int, half: int) -> str:
    p = int(rng.integers(0, split)) if half == 1 else int(rng.integers(split, len(tag)))
    return casegen.substitute(rng, tag, p)


def ladder_read(ts, rng, v: int, j: int, k_v: int, k_j: int, v_kind: int = 1, v_sub_half: int = 2, j_kind: int = 1,
                j_sub_half: int = 2, vdel: int = 0, jdel: int = 0, ins: int = 4):
    """One sense-frame read: [k_v V half tags of kind v_kind, two bases apart] [the V gene from its tag on, one
    substitution in half v_sub_half of the tag] [insert] [the J gene up to its tag's end, one substitution in half
    j_sub_half] [k_j J half tags of kind j_kind, two bases apart] [a few bases].  k = 0 leaves that side plain."""
    v_split, j_split = ts.half_splits
    vreg, jreg = ts.v_regions[v].upper(), ts.j_regions[j].upper()
    vt, jt = ts.v_tags[v], ts.j_tags[j]
    voff = len(vreg) - ts.v_jumps[v]
    fill = synth._rand_seq(rng, 64 + 2 * (k_v + k_j) + ins)          # every random base of the read, drawn at once
    lens = rng.integers(0, 7, size=3).tolist()
    if k_v:
        rungs = _ladder_halves(rng, ts.v_tags, v_split, v_kind, v, k_v)
        head = fill[:lens[0]] + "".join(h + fill[8 + 2 * i:10 + 2 * i] for i, h in enumerate(rungs))
        vtag = _sub_in_half(rng, vt, v_split, v_sub_half)
    else:
        head, vtag = fill[:20 + 3 * lens[0]], vt
    fill = fill[40 + 2 * k_v:]
    vpart = vtag + vreg[voff + len(vt):len(vreg) - vdel]
    if k_j:
        rungs = _ladder_halves(rng, ts.j_tags, j_split, j_kind, j, k_j)
        jtag = _sub_in_half(rng, jt, j_split, j_sub_half)
        tail = "".join(fill[2 * i:2 + 2 * i] + h for i, h in enumerate(rungs))
    else:
        jtag, tail = jt, jreg[ts.j_jumps[j] + len(jt):]
    fill = fill[2 * k_j:]
    jpart = jreg[jdel:ts.j_jumps[j]] + jtag
    return head + vpart + fill[:ins] + jpart + tail + fill[ins:ins + 3 + lens[1]]


def decoy_ladder(ts, rng, n: int, ks=LADDER_KS):
    """n ladder reads and their marks (k_v, k_j: the rungs on either side, 0 for none).  A third carry the ladder on
    the V side, a third on the J side, a third on both.  The ladder's kind of half and the half of the tag that takes
    the substitution are drawn independently: where they differ the tag's own hit is the last (V) or first (J) of
    k + 1 hits of one kind; where both are half 1 the reference finds half-1 hits only among the rungs and gives up
    (found...1not...2); where both are half 2 the tag's half-1 hit is alone and the rungs are never consulted."""
    reads, marks = [], np.zeros(n, dtype=MARKS_DTYPE)
    side = np.arange(n) % 3
    k_v = np.where(side != 1, rng.choice(ks, size=n), 0).tolist()
    k_j = np.where(side != 0, rng.choice(ks, size=n), 0).tolist()
    v, j = rng.integers(0, len(ts.v_tags), size=n).tolist(), rng.integers(0, len(ts.j_tags), size=n).tolist()
    kinds = rng.integers(1, 3, size=(n, 4)).tolist()
    vdel, jdel, ins = (rng.integers(0, hi, size=n).tolist() for hi in (6, 9, 9))
    for r in range(n):
        reads.append(ladder_read(ts, rng, v[r], j[r], k_v[r], k_j[r], *kinds[r], vdel[r], jdel[r], ins[r]))
        marks[r] = (v[r], j[r], False, False, k_v[r], k_j[r])
    return reads, marks


def half_hits(ot, read: str):
    """What the oracle's findall sees on a frame read: the number of hits of (V half 1, V half 2, J half 1, J half 2)."""
    return tuple(len(ot.findall(g, w, read)) for g in (0, 1) for w in (1, 2))


# --------------------------------------------------------------------------------------------------------------
# how contested a settled record is
# --------------------------------------------------------------------------------------------------------------

def is_contested(ts, frame_read: str, record):
    """(number of V tags, number of J tags) within Hamming 1 of the windows the record settled on; the read in the
    frame the record's positions count in.  (0, 0) for a read that was not decombined."""
    if int(record["status"]) != 0:
        return 0, 0
    lv = len(ts.v_tags[0])
    wv = frame_read[int(record["v_start"]):int(record["v_start"]) + lv]
    return (sum(hamming(wv, t) <= 1 for t in ts.v_tags),
            max(sum(hamming(frame_read[s:s + len(t)], t) <= 1 for t in ts.j_tags if s >= 0) for s in _j_starts(ts, int(record["j_end"]))))


def _j_starts(ts, j_end: int):
    """Where the J tag's window may start for a record's j_end: a full-tag or half-2 hit ends at the tag's end, a
    half-1 hit at its start + 2 * j_half_split (decombine.py:450-454), which is the tag's end for 10 + 10 tags only."""
    return sorted({j_end - len(ts.j_tags[0]), j_end - 2 * ts.half_splits[1]})


def _near(tags, windows) -> np.ndarray:
    t = np.frombuffer("".join(tags).encode(), dtype=np.uint8).reshape(len(tags), -1)
    w = np.frombuffer("".join(windows).encode("latin-1"), dtype=np.uint8).reshape(len(windows), -1)
    return ((w[:, None, :] != t[None, :, :]).sum(axis=2) <= 1).sum(axis=1)


def contested_counts(ts, frame_reads, records):
    """is_contested over a batch: two int arrays (0 where the read was not decombined)."""
    lv, lj = len(ts.v_tags[0]), len(ts.j_tags[0])
    ok = np.nonzero(records["status"] == 0)[0]
    nv, nj = np.zeros(len(records), dtype=np.int64), np.zeros(len(records), dtype=np.int64)
    if len(ok):
        vs, je = records["v_start"][ok].tolist(), records["j_end"][ok].tolist()
        wv = [frame_reads[i][s:s + lv].ljust(lv, "#") for i, s in zip(ok.tolist(), vs)]
        nv[ok] = _near(ts.v_tags, wv)
        for shift in sorted({lj, 2 * ts.half_splits[1]}):
            wj = [frame_reads[i][e - shift:e - shift + lj].ljust(lj, "#") if e >= shift else "#" * lj for i, e in zip(ok.tolist(), je)]
            nj[ok] = np.maximum(nj[ok], _near(ts.j_tags, wj))
    return nv, nj


def contest_report(ts, reads, marks, orec, ocnt, counter_names) -> dict:
    """The figures behind the conditions a contested workload has to meet, from the ORACLE's records of the sense
    reads in the forward frame and the generator's marks."""
    nv, nj = contested_counts(ts, reads, orec)
    ok = orec["status"] == 0
    mv, mj = marks["contested_v"] & ok, marks["contested_j"] & ok
    cv, cj = mv & (nv >= 2), mj & (nj >= 2)
    own = orec["v"] == marks["src_v"]
    rep = {"reads": len(reads), "decombined": int(ok.sum()), "marked_v_decombined": int(mv.sum()), "contested_v": int(cv.sum()),
           "marked_j_decombined": int(mj.sum()), "contested_j": int(cj.sum()),
           "v_won_by_source": int((cv & own).sum()), "v_won_by_other": int((cv & ~own).sum())}
    for k in ("verr1", "verr2", "jerr1", "jerr2"):
        rep[k] = int(ocnt[counter_names.index(k)])
    return rep


def assert_contest_conditions(rep: dict, scale: float = 1.0):
    """The conditions at 60 000 reads times `scale` (the counts scale with the workload, the shares do not)."""
    assert rep["contested_v"] >= 0.95 * rep["marked_v_decombined"], rep
    assert rep["v_won_by_source"] >= 0.30 * rep["contested_v"] and rep["v_won_by_other"] >= 0.30 * rep["contested_v"], rep
    assert rep["contested_v"] >= 10_000 * scale and rep["contested_j"] >= 3_000 * scale, rep
    for k in ("verr1", "verr2", "jerr1", "jerr2"):
        assert rep[k] > 1_000 * scale, rep
