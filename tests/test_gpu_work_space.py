"""The work space of every device entry that takes one: dcrx_merge_parents_device, dcrx_cdr3_device, dcrx_cdr3_neighbours_device
(Hamming and Levenshtein), dcrx_downsample_device, dcrx_cdr3_match_device (Hamming and Levenshtein),
dcrx_cdr3_match_weighted_device, dcrx_cdr3_neighbours_weighted_device, dcrx_cdr3_motifs_device, dcrx_cdr3_motif_members_device and
dcrx_cdr3_groups_device.  An entry promises to stay inside its *_work_bytes and to give a result that does not depend on what the
memory held before, so each runs in exactly that many bytes, 4096 guard bytes of 0xA5 behind them, under three states of the work
space: filled with 0x00 (a counter or table the entry forgot to zero goes unseen here alone), filled with 0xFF (a buffer it forgot
to set to all-ones goes unseen here alone), and left over — a larger case of the same entry has run over the same memory first, as
in a caller's recycled arena.  Under each state the guard stays untouched and the outputs are those of a call with a MiB to spare
and those of the stage's contract helper, written in Python; one byte less is refused with DCRX_E_INVALID.  Every output array is
exactly as long as include/dcrx.h says, with 64 bytes of 0xA5 behind it that stay, and so do the slots behind what an entry says it
writes.  Sizes 1 and 257 (and 0 where the entry takes it): 257 is one past a block, and its 1-, 4- and 8-byte columns do not fill
their 256-byte slot, so a buffer carved with the wrong element size runs into its neighbour or past the end."""
import ctypes
import functools
import random

import numpy as np
import pytest

from decombinator_amd import _native as nat
from decombinator_amd import synth, translate
from decombinator_amd.match import spans
from tests import cdr3_lev_util as clu
from tests import cdr3_match_util as cmu
from tests import cdr3_network_util as cnu
from tests import cdr3_wmatch_util as wu
from tests import cdr3_wnet_util as nu
from tests import clonotype_util as cu
from tests import motif_groups_util as gu
from tests import motif_util as mu
from tests import nbc_merge_util as nm
from tests import rarefy_util as ru

pytestmark = pytest.mark.gpu

E_INVALID = -1
GUARD, SPARE, TAIL = 4096, 1 << 20, 64
SIZES = [1, 257]
STATES = ("0x00", "0xFF", "left over")


def _fill(buf, at, value, count):
    if count:
        nat.check(nat.lib().dcrx_memset_device(buf.ptr + at, value, count))


def _peek(buf, at, count):
    out = np.zeros(count, np.uint8)
    nat.check(nat.lib().dcrx_memcpy_d2h(out.ctypes.data, buf.ptr + at, count))
    return out


class _Out:
    """An output array of exactly `count` entries, as include/dcrx.h documents it, with TAIL bytes behind it; 0xA5 all over
    before the call."""

    def __init__(self, dtype, count):
        self.dtype, self.count = np.dtype(dtype), int(count)
        self.bytes = self.count * self.dtype.itemsize
        self.buf = nat.DeviceBuffer.from_host(np.full(self.bytes + TAIL, 0xA5, np.uint8))
        self.ptr = self.buf.ptr

    def read(self, written=None):
        """The entries (the first `written` of them: the others have stayed as they were), the tail checked."""
        raw = self.buf.to_host(np.uint8, self.bytes + TAIL)
        assert (raw[self.bytes:] == 0xA5).all(), "written behind an output array"
        kept = self.bytes if written is None else int(written) * self.dtype.itemsize
        assert kept <= self.bytes and (raw[kept:self.bytes] == 0xA5).all(), "written behind what the entry says it writes"
        return raw[:kept].view(self.dtype).copy()


def _device(a):
    return nat.DeviceBuffer.from_host(np.ascontiguousarray(a))


def _text(text: bytes):
    return nat.DeviceBuffer.from_host(np.frombuffer(text + b"\0", np.uint8))


def _guarded(run, work_bytes, before, check, refused=True):
    """run(d_work, size) makes the entry's calls on the null stream, synchronises and returns the outputs as arrays; before is
    (run, work_bytes) of a larger case of the same entry; check(outputs) holds them against the stage's contract.  The call in
    exactly work_bytes under each state of the work space — the guard, the contract —, then the call with a MiB to spare — the
    contract, and every state's outputs are its outputs byte for byte — and the refusal.  refused False: the header says that
    the case launches nothing and does not look at the work space."""
    assert work_bytes > 0
    big_run, big_bytes = before

    def checked(outputs, what):
        try:
            check(outputs)
        except AssertionError as e:
            raise AssertionError(f"the work space: {what}: {e}") from e
        return outputs
    tight = {}
    for state in STATES:
        if state == "left over":
            d_work = nat.DeviceBuffer(max(big_bytes, work_bytes + GUARD))
            big_run(d_work, big_bytes)
        else:
            d_work = nat.DeviceBuffer(work_bytes + GUARD)
            _fill(d_work, 0, 0xFF if state == "0xFF" else 0x00, work_bytes)
        _fill(d_work, work_bytes, 0xA5, GUARD)
        nat.synchronize()
        tight[state] = run(d_work, work_bytes)
        assert (_peek(d_work, work_bytes, GUARD) == 0xA5).all(), state
        checked(tight[state], state)
    roomy = checked(run(nat.DeviceBuffer(work_bytes + SPARE), work_bytes + SPARE), "a MiB to spare")
    for state in STATES:
        assert len(tight[state]) == len(roomy)
        for k, (a, b) in enumerate(zip(tight[state], roomy)):
            assert a.dtype == b.dtype and np.array_equal(a, b), (state, k)
    if refused:
        with pytest.raises(nat.DcrxError) as e:
            run(d_work, work_bytes - 1)
        assert e.value.code == E_INVALID


# ---- dcrx_merge_parents_device ----

def _merge_table(n):
    """n entries over a few (v, j) buckets in rank order: parents with a child one substitution away and a hundredth of the reads."""
    rng = np.random.default_rng(40 + n)
    entries, seen = [], set()
    while len(entries) < n:
        src = "".join(rng.choice(list("ACGT"), size=24))
        p = int(rng.integers(0, 24))
        sub = src[:p] + "ACGT"[("ACGT".index(src[p]) + 1) % 4] + src[p + 1:]
        if src in seen or sub in seen:
            continue
        seen |= {src, sub}
        v, j, k = int(rng.integers(0, 3)), int(rng.integers(0, 3)), len(entries)
        entries.append((v, j, 4, 3, src, int(rng.integers(2000, 9000)), k))
        if len(entries) < n:
            entries.append((v, j, 4, 3, sub, int(rng.integers(1, 100)), k + 1))
    return nm.ranked(entries)


def _merge_run(t, counted, n):
    bufs = [_device(counted[f]) for f in ("v", "j", "vdel", "jdel", "count", "ins_off")]
    text = np.frombuffer(counted["ins_text"], np.uint8)
    d_text = _device(text)

    def run(d_work, size):
        d_parent, d_reach = _Out(np.uint32, n), _Out(np.uint8, n)
        nat.merge_parents_device(t, n, *bufs, d_text, len(text), 1, 10, d_parent, d_reach, d_work, size)
        nat.synchronize()
        return d_parent.read(), d_reach.read()
    return run, int(nat.lib().dcrx_merge_work_bytes(n))


@pytest.mark.parametrize("n", SIZES)
def test_merge_parents_device(n):
    ts = synth.config_tagset(2)
    t = nat.Tables(ts.v_tags, ts.v_jumps, ts.v_regions, ts.j_tags, ts.j_jumps, ts.j_regions, *ts.half_splits)
    counted = _merge_table(n)
    _, wstats, wroot = nm.expected_merge(counted, ts, 1, 10)
    assert wstats["merged"] == n // 2 and wstats["out_of_reach"] == 0

    def check(outputs):
        parent, reach = outputs
        assert np.array_equal(nm.roots_of(parent), wroot) and reach.all()
    _guarded(*_merge_run(t, counted, n), before=_merge_run(t, _merge_table(1500), 1500), check=check)


# ---- dcrx_cdr3_device ----

def _cdr3_run(genes, tab):
    n, text = len(tab["v"]), tab["ins_text"]
    d = [_device(tab[k]) for k in ("v", "j", "vdel", "jdel", "ins_off")]
    d_text = _text(text)

    def run(d_work, size):
        # sized first (no arena), then written into an arena of exactly that size
        d_rows, d_need = _Out(nat.CLONO_ROW_DTYPE, n), _Out(np.uint64, 1)
        nat.cdr3_device(genes, n, *d, d_text, len(text), d_rows, None, 0, d_need, d_work, size)
        nat.synchronize()
        need = int(d_need.read()[0])
        d_arena = _Out(np.uint8, need)
        nat.cdr3_device(genes, n, *d, d_text, len(text), d_rows, d_arena, need, d_need, d_work, size)
        nat.synchronize()
        return d_rows.read(), d_arena.read(), d_need.read()
    return run, nat.clono_work_bytes(n, len(text))


@pytest.mark.parametrize("n", SIZES)
def test_cdr3_device(n):
    G = cu.golden_genes()
    all_rows = cu.table_rows(cu.random_table(G, 400, seed=3))
    tab = cu.table(all_rows[:n])
    assert len(tab["v"]) == n and len(all_rows) == 400
    genes = translate._clono_genes(G)

    def check(outputs):
        rows, arena, _ = outputs
        seen = cu.assert_rows_equal_batch(G, tab, rows, arena.tobytes())
        assert sum(seen.values()) == n and (n == 1 or int((rows["flags"] & 1).sum()) > 20)
    _guarded(*_cdr3_run(genes, tab), before=_cdr3_run(genes, cu.table(all_rows)), check=check)


# ---- dcrx_cdr3_neighbours_device, dcrx_cdr3_neighbours_metric_device ----

def _neighbours_run(metric, n, seed):
    strings = (cnu.families if metric is None else clu.families_indel)(n, seed=seed, length=13)
    classes = [k % 3 for k in range(n)]
    off, text = cnu.node_text(strings)
    d_cls, d_off, d_text = _device(np.asarray(classes, dtype=np.uint32)), _device(off), _text(text)

    def run(d_work, size):
        # sized first (no adjacency), then written into one of exactly the need
        d_deg, d_adj_off, d_need = _Out(np.uint32, n), _Out(np.uint64, n + 1), _Out(np.uint64, 1)
        nat.cdr3_neighbours_device(n, d_cls, d_off, d_text, len(text), 2, d_deg, d_adj_off, None, 0, d_need, d_work, size, metric=metric)
        nat.synchronize()
        need = int(d_need.read()[0])
        d_adj = _Out(np.uint32, need)
        nat.cdr3_neighbours_device(n, d_cls, d_off, d_text, len(text), 2, d_deg, d_adj_off, d_adj, need, d_need, d_work, size, metric=metric)
        nat.synchronize()
        return d_deg.read(), d_adj_off.read(), d_adj.read(), d_need.read()
    return (run, nat.cdr3net_work_bytes(n, len(text), metric=metric)), classes, strings


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("metric", [None, "levenshtein"], ids=["hamming", "levenshtein"])
def test_cdr3_neighbours_device(metric, n):
    mine, classes, strings = _neighbours_run(metric, n, 9)
    want, st = (cnu.expected_network if metric is None else clu.expected_lev_network)(classes, strings, [1] * n, 2)
    assert n == 1 or st["edges"] > 20

    def check(outputs):
        deg, adj_off, adj, need = outputs
        assert len(adj) == 2 * st["edges"] == int(need[0])
        assert np.array_equal(deg, want["degree"]) and np.array_equal(adj_off, want["adj_off"]) and np.array_equal(adj, want["adj"])
    _guarded(*mine, before=_neighbours_run(metric, 1500, 10)[0], check=check)


# ---- dcrx_downsample_device ----

def _downsample_run(S, m):
    """Per sample a depth below its reads, but the last of three, which keeps every read."""
    rng = np.random.default_rng(7 * m + S)
    samples = sorted(int(k * S // m) for k in range(m))
    weights = [int(x) for x in rng.integers(1, 41, size=m)]
    reads = [sum(w for s, w in zip(samples, weights) if s == k) for k in range(S)]
    depths = [reads[k] // 3 for k in range(S)]
    if S == 3:
        depths[2] = reads[2] + 5
    inputs = [_device(np.asarray(a, dt)) for a, dt in ((samples, np.uint32), (weights, np.uint64), (depths, np.uint64))]

    def run(d_work, size):
        outs = [_Out(np.uint64, k) for k in (m, S, S, S)]
        nat.downsample_device(S, m, *inputs, 17, *outs, d_work, size)
        nat.synchronize()
        return [b.read() for b in outs]
    return (run, nat.downsample_work_bytes(m, S)), samples, weights, depths


@pytest.mark.parametrize("S,m", [(1, 1), (1, 257), (3, 257)])
def test_downsample_device(S, m):
    mine, samples, weights, depths = _downsample_run(S, m)
    want = ru.expected_downsample(samples, weights, S, depths, 17)

    def check(outputs):
        got = dict(zip(ru.OUTPUTS, outputs))
        ru.assert_same(got, want)
        ru.assert_sums(got, samples)
    _guarded(*mine, before=_downsample_run(3, 1500)[0], check=check)


# ---- dcrx_cdr3_match_device, dcrx_cdr3_match_weighted_device ----

M_Q = [0, 1, 257]


@functools.lru_cache(maxsize=None)
def _match_case(indel: bool, m_q: int) -> cmu.Case:
    """300 targets in three classes and m_q queries, each a target's string after 0 to 3 edits (substitutions; with `indel`
    insertions and deletions too), three in four of them in that target's class."""
    targets = (clu.families_indel if indel else cnu.families)(300, seed=41, length=13)
    t_classes = [k % 3 for k in range(300)]
    rnd = random.Random(1000 * m_q + indel)
    q_classes, queries = [], []
    for _ in range(m_q):
        j, k = rnd.randrange(300), rnd.choice((0, 1, 1, 2, 3))
        queries.append(clu.edit(targets[j], k, rnd) if indel else cnu.mutate(targets[j], k, rnd))
        q_classes.append(t_classes[j] if rnd.random() < 0.75 else (t_classes[j] + 1) % 3)
    return cmu.Case(t_classes, targets, q_classes, queries)


def _match_run(index, case, call, work_bytes, dist):
    """call(m_q, d_cls, d_off, d_text, text_bytes, d_deg, d_hit_off, d_hit, d_dist, cap, d_need, d_work, size) is the entry under
    one metric; the two calls of the contract: sized with no hit buffer, then written into exactly the need."""
    _, (qc, off, text, _) = cmu.native_args(case)
    m = len(qc)
    d_cls, d_off, d_text = _device(qc), _device(off), _text(text)

    def run(d_work, size):
        d_deg, d_hit_off, d_need = _Out(np.uint32, m), _Out(np.uint64, m + 1), _Out(np.uint64, 1)
        call(m, d_cls, d_off, d_text, len(text), d_deg, d_hit_off, None, None, 0, d_need, d_work, size)
        nat.synchronize()
        need = int(d_need.read()[0])
        d_hit, d_dist = _Out(np.uint32, need), _Out(np.uint32, need if dist else 0)
        call(m, d_cls, d_off, d_text, len(text), d_deg, d_hit_off, d_hit, d_dist if dist else None, need, d_need, d_work, size)
        nat.synchronize()
        return d_deg.read(), d_hit_off.read(), d_hit.read(), d_dist.read(), d_need.read()
    return run, work_bytes(m, len(text))


@pytest.mark.parametrize("m_q", M_Q)
@pytest.mark.parametrize("metric", cmu.METRICS)
def test_cdr3_match_device(metric, m_q):
    indel = metric == "levenshtein"
    case = _match_case(indel, m_q)
    want = cmu.Reference(case).expected(2, metric)
    assert m_q < 257 or want["stats"]["hits"] > 20

    def check(outputs):
        deg, hit_off, hit, _, need = outputs
        assert int(need[0]) == want["stats"]["hits"] == len(hit)
        assert np.array_equal(deg, want["degree"]) and np.array_equal(hit_off, want["hit_off"]) and np.array_equal(hit, want["hit"])
    index = nat.Cdr3Index(*cmu.native_args(case)[0])
    try:
        def call(m, d_cls, d_off, d_text, text_bytes, d_deg, d_hit_off, d_hit, _, cap, d_need, d_work, size):
            nat.cdr3_match_device(index, m, d_cls, d_off, d_text, text_bytes, 2, d_deg, d_hit_off, d_hit, cap, d_need, d_work, size, None, metric)
        work_bytes = lambda m, text_bytes: nat.cdr3_match_work_bytes(m, text_bytes, metric)
        # (no query: the header has the entry zero its outputs and look at nothing else, the work space included)
        _guarded(*_match_run(index, case, call, work_bytes, False), before=_match_run(index, _match_case(indel, 1500), call, work_bytes, False),
                 check=check, refused=m_q > 0)
    finally:
        index.close()


@pytest.mark.parametrize("m_q", M_Q)
def test_cdr3_match_weighted_device(m_q):
    case, cost, R = _match_case(True, m_q), wu.default_cost(), 24
    want = wu.expected_numpy(case, cost, R)
    assert m_q < 257 or (want["stats"]["hits"] > 20 and len(set(want["hit_dist"].tolist())) > 3)

    def check(outputs):
        deg, hit_off, hit, dist, need = outputs
        assert int(need[0]) == want["stats"]["hits"] == len(hit) == len(dist)
        assert np.array_equal(deg, want["degree"]) and np.array_equal(hit_off, want["hit_off"])
        assert np.array_equal(hit, want["hit"]) and np.array_equal(dist, want["hit_dist"])
    index = nat.Cdr3Index(*cmu.native_args(case)[0])
    try:
        def call(m, d_cls, d_off, d_text, text_bytes, d_deg, d_hit_off, d_hit, d_dist, cap, d_need, d_work, size):
            nat.cdr3_match_weighted_device(index, m, d_cls, d_off, d_text, text_bytes, cost, R, d_deg, d_hit_off, d_hit, d_dist, cap, d_need,
                                           d_work, size)
        _guarded(*_match_run(index, case, call, nat.cdr3_match_weighted_work_bytes, True),
                 before=_match_run(index, _match_case(True, 1500), call, nat.cdr3_match_weighted_work_bytes, True), check=check, refused=m_q > 0)
    finally:
        index.close()


# ---- dcrx_cdr3_neighbours_weighted_device ----

def _wnet_run(nodes, cost, R):
    m = len(nodes)
    off, text = cnu.node_text(nodes.strings)
    d_cls, d_off, d_text = _device(np.asarray(nodes.classes, dtype=np.uint32)), _device(off), _text(text)

    def run(d_work, size):
        # sized first, then written, the distances beside the neighbours
        d_deg, d_adj_off, d_need = _Out(np.uint32, m), _Out(np.uint64, m + 1), _Out(np.uint64, 1)
        nat.cdr3_neighbours_weighted_device(m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_adj_off, None, None, 0, d_need, d_work, size)
        nat.synchronize()
        need = int(d_need.read()[0])
        d_adj, d_dist = _Out(np.uint32, need), _Out(np.uint32, need)
        nat.cdr3_neighbours_weighted_device(m, d_cls, d_off, d_text, len(text), cost, R, d_deg, d_adj_off, d_adj, d_dist, need, d_need, d_work,
                                            size)
        nat.synchronize()
        return d_deg.read(), d_adj_off.read(), d_adj.read(), d_dist.read(), d_need.read()
    return run, nat.cdr3net_weighted_work_bytes(m, len(text))


@pytest.mark.parametrize("m", SIZES)
def test_cdr3_neighbours_weighted_device(m):
    """The strings of nu.tiles (three lengths mixed), the ranks dealt out over three classes seven at a time."""
    nodes, cost, R = nu.Nodes([7 + i // 7 % 3 for i in range(m)], [nu.code(i) for i in range(m)]), wu.default_cost(), 24
    want, stats = nu.expected_numpy(nodes, cost, R)
    assert m == 1 or (stats["edges"] > 20 and len(set(want["adj_dist"].tolist())) > 3)
    big, big_cost, big_R, _ = nu.constructed()["tiles_1500"]

    def check(outputs):
        deg, adj_off, adj, dist, need = outputs
        assert int(need[0]) == 2 * stats["edges"] == len(adj)
        assert np.array_equal(deg, want["degree"]) and np.array_equal(adj_off, want["adj_off"])
        assert np.array_equal(adj, want["adj"]) and np.array_equal(dist, want["adj_dist"])
    _guarded(*_wnet_run(nodes, cost, R), before=_wnet_run(big, big_cost, big_R), check=check)


# ---- dcrx_cdr3_motifs_device ----

KS, TRIM = (2, 3, 4), (3, 3)


def _motifs_run(sample, background, resamples, seed, cap):
    n, m = len(sample), len(background)
    inputs = [_device(np.frombuffer(x, np.uint8) if isinstance(x, bytes) else x) for x in spans(list(sample)) + spans(list(background))]

    def run(d_work, size):
        outs = [_Out(dt, cap) for _, dt in nat.CDR3_MOTIF_OUTPUTS]
        d_need, d_stats = _Out(np.uint64, 1), _Out(np.uint64, len(nat.CDR3_MOTIF_STATS))
        nat.cdr3_motifs_device(n, inputs[0], inputs[1], m, inputs[2], inputs[3], KS, TRIM, 1, resamples, seed, cap, *outs, d_need, d_stats,
                               d_work, size)
        nat.synchronize()
        need = d_need.read()
        return [b.read(min(int(need[0]), cap)) for b in outs] + [need, d_stats.read()]
    return run, nat.cdr3_motifs_work_bytes(n, m, resamples)


@pytest.mark.parametrize("n,m,chunks,cap", [(0, 50, 3, None), (30, 0, 0, None), (1, 40, 9, None), (257, 600, None, None), (257, 600, None, 40)])
def test_cdr3_motifs_device(n, m, chunks, cap):
    """chunks None: one resample more than a chunk holds, so the loop runs a full chunk — `list` and `plane` at their whole carve —
    and a chunk of one.  cap None: the need."""
    assert ctypes.sizeof(nat.Cdr3MotifStatsC) == 8 * len(nat.CDR3_MOTIF_STATS)
    resamples = mu.constant("MAX_CHUNK") + 1 if chunks is None else chunks
    assert chunks is not None or mu.chunk_of(n) == mu.constant("MAX_CHUNK")
    pool = mu.random_units(700, 21, 8, 14)
    sample, background = list(pool[:n]), list(pool[100:100 + m])
    whole = mu.expected_motifs(sample, background, KS, TRIM, 1, resamples, 1)
    cap = whole["need"] if cap is None else cap
    assert cap <= whole["need"] and (n < 257 or whole["need"] > 40)
    want = mu.expected_motifs(sample, background, KS, TRIM, 1, resamples, 1, cap)
    other = mu.random_units(2400, 22, 8, 14)
    assert [name for name, _ in nat.CDR3_MOTIF_OUTPUTS] == list(mu.FIELDS)

    def check(outputs):
        *rows, need, stats = outputs
        mu.assert_same(dict(zip(mu.FIELDS, rows), need=int(need[0]), stats={k: int(v) for k, v in zip(nat.CDR3_MOTIF_STATS, stats)}), want)
        assert all(len(r) == cap for r in rows)
    _guarded(*_motifs_run(sample, background, resamples, 1, cap), before=_motifs_run(other[:400], other[400:], 70, 2, 400 * 90), check=check)


# ---- dcrx_cdr3_motif_members_device ----

def _members_run(units, selected, cap):
    n, S = len(units), len(selected)
    off, text = spans(list(units))
    d_off, d_text = _device(np.asarray(off, np.uint64)), _text(bytes(text))
    d_sel_k, d_sel_code = (_device(np.array([kc[i] for kc in selected], np.uint32)) for i in (0, 1))

    def run(d_work, size):
        d_n_motifs, d_mem_off, d_mem, d_need = _Out(np.uint32, n), _Out(np.uint64, S + 1), _Out(np.uint32, cap), _Out(np.uint64, 1)
        nat.cdr3_motif_members_device(n, d_off, d_text, (2, 3), TRIM, S, d_sel_k, d_sel_code, cap, d_n_motifs, d_mem_off, d_mem, d_need, d_work, size)
        nat.synchronize()
        need = d_need.read()
        return d_n_motifs.read(), d_mem_off.read(), d_mem.read(min(int(need[0]), cap)), need
    return run, nat.cdr3_motif_members_work_bytes(n, cap)


@functools.lru_cache(maxsize=None)
def _members_before():
    """400 units with the motifs two of them hold, and the members' number."""
    units = mu.random_units(400, 23, 8, 14)
    selected = gu.motifs_held(units, (2, 3), TRIM)
    return units, selected, gu.expected_members(list(units), (2, 3), TRIM, selected)["need"]


@pytest.mark.parametrize("n,held_by", [(1, 1), (257, 2), (257, None)], ids=["1", "257", "257-no-motif"])
def test_cdr3_motif_members_device(n, held_by):
    """The selected motifs are those `held_by` of the units hold at least (None: no motif is selected); cap 0 (a counting call),
    one below the need and the need: the sort runs over cap + n slots."""
    units = list(mu.random_units(700, 21, 8, 14)[:n])
    selected = gu.motifs_held(units, (2, 3), TRIM, held_by) if held_by else []
    whole = gu.expected_members(units, (2, 3), TRIM, selected)
    need = whole["need"]
    assert (need == 0) == (held_by is None) and (n == 1 or held_by is None or need > 300)
    for cap in sorted({0, max(need - 1, 0), need}):
        want = gu.expected_members(units, (2, 3), TRIM, selected, cap)

        def check(outputs):
            n_motifs, mem_off, mem, got_need = outputs
            gu.assert_same_members({"n_motifs": n_motifs, "mem_off": mem_off, "mem": mem, "need": int(got_need[0])}, want)
            assert len(mem) == cap and len(mem_off) == len(selected) + 1
        _guarded(*_members_run(units, selected, cap), before=_members_run(*_members_before()), check=check)


# ---- dcrx_cdr3_groups_device ----

def _groups_run(n, weights, adjacency, rows):
    S = len(rows)
    (adj_off, adj), (mem_off, mem) = gu.csr(adjacency), gu.csr(rows)
    d_weight, d_adj_off = _device(np.array(weights, np.uint64)), _device(adj_off)
    d_adj, d_mem_off, d_mem = _device(adj) if len(adj) else None, _device(mem_off) if S else None, _device(mem) if len(mem) else None

    def run(d_work, size):
        outs = [_Out(np.uint32, n), _Out(np.uint32, n), _Out(np.uint32, n), _Out(np.uint64, n)]
        d_groups = _Out(np.uint32, 1)
        rounds = nat.cdr3_groups_device(n, d_weight, d_adj_off, d_adj, len(adj), S, d_mem_off, d_mem, len(mem), *outs, d_groups, d_work, size)
        nat.synchronize()
        groups = d_groups.read()
        return [outs[0].read()] + [b.read(int(groups[0])) for b in outs[1:]] + [groups, np.array([rounds], np.uint32)]
    return run, nat.cdr3_groups_work_bytes(n, S)


@functools.lru_cache(maxsize=None)
def _groups_rows(n: int, first: int, last: int, at_least: int):
    """The member rows, over the first n units of the pool, of the 3-mers that `at_least` of the units first .. last - 1 hold."""
    pool = mu.random_units(400, 21, 8, 14)
    selected = gu.motifs_held(pool[first:last], (3,), TRIM, at_least)
    return gu.expected_members(list(pool[:n]), (3,), TRIM, selected)["rows"]


@pytest.mark.parametrize("shape", ["0", "1", "257-ring", "257-rows", "257-both"])
def test_cdr3_groups_device(shape):
    """No unit; one; 257 with an adjacency alone (every seventh unit linked to the next seventh), with member rows alone — the
    rows, over the 257, of the motifs that units 0 .. 329 hold: some are empty, some hold one unit — and with both."""
    n = int(shape.split("-")[0])
    rows = _groups_rows(257, 0, 330, 1) if shape in ("257-rows", "257-both") else []
    weights, adjacency, want = gu.groups_table(n, rows, ring=shape in ("257-ring", "257-both"))
    if rows:
        assert min(len(r) for r in rows) == 0 and any(len(r) == 1 for r in rows) and sum(len(r) > 1 for r in rows) > 20
    assert n < 257 or 1 < len(want["head"]) < n
    big_rows = _groups_rows(300, 0, 300, 2)

    def check(outputs):
        *per, groups, rounds = outputs
        assert int(groups[0]) == len(want["head"]) and (int(rounds[0]) >= 2) == (n == 257)
        for got, f in zip(per, ("group_of", "head", "units", "weight")):
            assert [int(x) for x in got] == want[f], f
    _guarded(*_groups_run(n, weights, adjacency, rows), before=_groups_run(300, *gu.groups_table(300, big_rows)[:2], big_rows), check=check)
