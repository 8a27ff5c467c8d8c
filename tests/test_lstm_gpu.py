"""GPU parity of the LSTM recurrence (csrc/lstm.hip: vqa_lstm_seq_fwd / vqa_lstm_seq_bwd) against tests/lstm_ref.py, and
the host logic of its hipGraph cache.

The reference is float64 with explicit BPTT and is tied to torch.nn.LSTM by tests/test_lstm_ref_cpu.py, which also shows
that the comparison made here rejects `t <= q_len`, swapped state slots in the reverse direction and a dropped pass-through
of dh.  Every output buffer is pre-filled with NaN and followed by a NaN guard tail; c_n lands inside a wider NaN matrix.
Afterwards everything the contract says is written must be finite, every guard untouched.

Exact checks: gate / dgates rows of an inactive (t, b) are 0.0; the state written for an inactive (t, b) has the bits of
the slot it was read from.  Parity: gates, Hs, Cs, c_n at 5e-6 and dgates, exit dh, exit dc at 2e-5 of max|ref| (the bounds
of tests/test_kernels_gpu.py), scaled by sqrt(T / 5) for T > 5: the per-step activation error (<= 3e-7 absolute) adds as
a random walk.  A plain float32 evaluation of the reference is 1e-7 .. 8e-7 from float64 on all of these up to B=130,
H=160, T=30, so the bounds are 15 - 60 times the format's own error.

Exit dh: vqa_lstm_seq_bwd leaves in dh the gradient w.r.t. the state that the FIRST processed time wrote (include/vqa_hip.h)
-- the last value BPTT multiplies into a cell -- not d loss / d h0, which would take one more W_hh product that no caller
needs.  The reference's `dh_first` is that quantity.
"""
import functools

import pytest
import torch

from tests import lstm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 96           # floats behind every buffer
CF_PAD = 4           # guard columns on either side of the c_n columns


def _ops():
    from dl_vqa_amd import ops
    return ops


def guarded(*shape):
    """(a NaN tensor of `shape`, the NaN tail that follows it in memory)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + GUARD,), NAN, device=DEV)
    return flat[:n].view(*shape), flat[n:]


def untouched(t):
    return bool(torch.isnan(t).all())


class Run:
    """Device buffers of one case (every direction), the calls, and the checks."""

    def __init__(self, q_len, dirs):
        self.src = dirs
        self.ndir = len(dirs)
        T, B, H4 = dirs[0]["xg"].shape
        self.T, self.B, self.H = T, B, H4 // 4
        H, Ta = self.H, T
        self.q_len = q_len.to(DEV)
        self.cf_ld = self.ndir * H + 2 * CF_PAD
        self.cf = torch.full((B, self.cf_ld), NAN, device=DEV)
        self.tails, self.d = [], []
        for k, s in enumerate(dirs):
            t = dict(reverse=s["reverse"], c_final=self.cf[:, CF_PAD + k * H:])
            for name, shape in (("w_hh", (4 * H, H)), ("xg", (Ta, B, 4 * H)), ("gates", (Ta, B, 4 * H)), ("Hs", (Ta + 1, B, H)),
                                ("Cs", (Ta + 1, B, H)), ("dgates", (Ta, B, 4 * H)), ("dh", (B, H)), ("dc", (B, H))):
                t[name], tail = guarded(*shape)
                self.tails.append((f"dir{k} {name}", tail))
            t["w_hh"].copy_(s["w_hh"])
            t["xg"][:T].copy_(s["xg"])
            self.d.append(t)
        self.reset()

    def reset(self, T=None):
        """NaN in every output, the initial state in its slot, the incoming gradients in dh / dc"""
        T = T or self.T
        self.cf.fill_(NAN)
        for t, s in zip(self.d, self.src):
            for name in ("gates", "Hs", "Cs", "dgates"):
                t[name].fill_(NAN)
            init = T if s["reverse"] else 0
            t["Hs"][init].copy_(s["h0"])
            t["Cs"][init].copy_(s["c0"])
            t["dh"].copy_(s["dh_n"])
            t["dc"].copy_(s["dc_n"])

    def fwd(self, use_graph, T=None):
        _ops().lstm_seq_fwd(self.d, self.q_len, self.B, T or self.T, self.H, cf_ld=self.cf_ld, use_graph=use_graph)

    def bwd(self, use_graph, T=None):
        _ops().lstm_seq_bwd(self.d, self.q_len, self.B, T or self.T, self.H, use_graph=use_graph)

    def got(self, k, T=None, backward=True):
        """outputs of direction k on the CPU, under the reference's names"""
        T, H, t = T or self.T, self.H, self.d[k]
        out = dict(gates=t["gates"][:T], Hs=t["Hs"][:T + 1], Cs=t["Cs"][:T + 1],
                   c_n=self.cf[:, CF_PAD + k * H:CF_PAD + (k + 1) * H])
        if backward:
            out.update(dgates=t["dgates"][:T], dh_first=t["dh"], dc0=t["dc"])
        return {n: v.detach().cpu().clone() for n, v in out.items()}

    def check_guards(self):
        H = self.H
        assert untouched(self.cf[:, :CF_PAD]) and untouched(self.cf[:, CF_PAD + self.ndir * H:]), "c_n guard columns written"
        for name, tail in self.tails:
            assert untouched(tail), f"the guard tail behind {name} was written"
        for t, s in zip(self.d, self.src):
            assert torch.equal(t["w_hh"].cpu(), s["w_hh"]) and torch.equal(t["xg"][:self.T].cpu(), s["xg"]), "an input changed"

    def check(self, refs, label, T=None, backward=True, emit=print):
        T = T or self.T
        for k, ref in enumerate(refs):
            got = self.got(k, T, backward)
            for name, v in got.items():
                assert bool(torch.isfinite(v).all()), f"{label} dir{k} {name}: unwritten / non-finite elements"
            bad = R.compare(got, ref, T, f"{label} dir{k}", emit=emit)
            assert not R.exact_violations(got, ref["active"], self.src[k]["reverse"])
            assert not bad, f"{label} dir{k}: {bad} beyond the bound"


@functools.lru_cache(maxsize=None)
def case(idx):
    """inputs and float64 references of R.CASES[idx], computed once for both launch modes"""
    q_len, dirs = R.case_inputs(idx)
    return q_len, dirs, [R.ref_of(q_len, d) for d in dirs]


def _label(idx):
    B, H, T, revs, state, dh_in = R.CASES[idx]
    return f"B{B} H{H} T{T} {''.join('R' if r else 'F' for r in revs)}{' h0' if state else ''}{' dh' if dh_in else ''}"


@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[_label(i).replace(" ", "-") for i in range(len(R.CASES))])
def test_sequence_against_float64(idx, graph):
    ops = _ops()
    q_len, dirs, refs = case(idx)
    run = Run(q_len, dirs)
    torch.cuda.synchronize()                     # a graph build may evict a cached graph: nothing is in flight
    before = ops.lstm_graph_stats()
    for rep in range(2 if graph else 1):         # the second call replays the graphs the first one built
        run.reset()
        run.fwd(graph)
        run.bwd(graph)
    torch.cuda.synchronize()
    after = ops.lstm_graph_stats()
    if graph:
        assert after[0] - before[0] == 2 and after[1] - before[1] == 2 and after[2] == before[2], (before, after)
    else:
        assert after[:3] == before[:3], (before, after)
    run.check_guards()
    run.check(refs, _label(idx) + (" graph" if graph else " plain"))


# ----------------------------------------------------------------------------- the graph cache (host logic of run_sequence)
def _delta(a, b):
    return tuple(y - x for x, y in zip(a[:3], b[:3]))      # (replays, builds, plain fallbacks)


def test_graph_cache_moved_buffers_fall_back_to_plain_launches():
    """A caller whose buffers move on every call: 8 builds, then plain launches; a replay resets the streak.  The shape
    (B=9, H=32, T=3, one reverse direction) is used nowhere else, so both miss streaks start at 0."""
    ops = _ops()
    q_len, dirs = R.make_case(9, 32, 3, (True,), True, True, seed=77)
    refs = [R.ref_of(q_len, d) for d in dirs]
    sets = [Run(q_len, dirs) for _ in range(12)]             # 12 live buffer sets: 12 distinct pointer sets
    deltas = []
    for i, run in enumerate(sets):
        torch.cuda.synchronize()
        s0 = ops.lstm_graph_stats()
        run.fwd(True)
        s1 = ops.lstm_graph_stats()
        run.bwd(True)
        s2 = ops.lstm_graph_stats()
        deltas.append((_delta(s0, s1), _delta(s1, s2)))
    print(f"[graph] 12 moved buffer sets, (replays, builds, plain) per call, fwd / bwd: {deltas}")
    assert deltas[:8] == [((0, 1, 0), (0, 1, 0))] * 8 and deltas[8:] == [((0, 0, 1), (0, 0, 1))] * 4, deltas
    torch.cuda.synchronize()
    for i, run in enumerate(sets):
        run.check_guards()
        run.check(refs, f"moved set {i}", emit=print if i in (0, 11) else None)
    # a cached set replays (and resets the streak) ...
    rep = sets[7]
    rep.reset()
    torch.cuda.synchronize()
    s0 = ops.lstm_graph_stats()
    rep.fwd(True)
    rep.bwd(True)
    s1 = ops.lstm_graph_stats()
    assert _delta(s0, s1) == (2, 0, 0), (s0, s1)
    # ... so a fresh set builds again
    fresh = Run(q_len, dirs)
    torch.cuda.synchronize()
    fresh.fwd(True)
    fresh.bwd(True)
    s2 = ops.lstm_graph_stats()
    print(f"[graph] replay of a cached set {_delta(s0, s1)}, fresh set after it {_delta(s1, s2)}")
    assert _delta(s1, s2) == (0, 2, 0), (s1, s2)
    torch.cuda.synchronize()
    for label, run in (("replayed set", rep), ("fresh set", fresh)):
        run.check_guards()
        run.check(refs, label)


def test_graph_cache_evicts_least_recently_used():
    """One buffer set sized for T = 34, called with T = 1 .. 34: 34 keys for a cache of 32.  Forward only (one key per T);
    B=7, H=32, both directions."""
    ops = _ops()
    TMAX, B, H = 34, 7, 32
    q_len, dirs = R.make_case(B, H, TMAX, (False, True), True, False, seed=78)
    run = Run(q_len, dirs)

    @functools.lru_cache(maxsize=None)
    def refs(T):
        return [R.lstm_dir_ref(d["xg"][:T], d["w_hh"], q_len, d["reverse"], d["h0"], d["c0"]) for d in dirs]

    def call(T):
        run.reset(T)
        torch.cuda.synchronize()                 # the build below may destroy a cached graph
        s0 = ops.lstm_graph_stats()
        run.fwd(True, T)
        torch.cuda.synchronize()
        s1 = ops.lstm_graph_stats()
        assert s1[3] <= 32, s1
        run.check(refs(T), f"T={T} of {TMAX}", T=T, backward=False)
        return _delta(s0, s1), s1[3]

    sizes = []
    for T in range(1, TMAX + 1):
        d, n = call(T)
        assert d == (0, 1, 0), (T, d)
        sizes.append(n)
    assert sizes[-1] == 32 and sizes[-2] == 32, sizes        # 34 inserts: full whatever was cached before
    again, n1 = call(TMAX)
    evicted, n2 = call(1)                                     # T = 1 and 2 were the least recently used of the 34
    print(f"[graph] eviction: cached graphs after each of 34 keys {sizes}; T=34 again {again}; evicted T=1 again {evicted}; "
          f"cached {n1} -> {n2}")
    assert again == (1, 0, 0) and evicted == (0, 1, 0) and n1 == 32 and n2 == 32
    run.check_guards()


# ----------------------------------------------------------------------------- the caller captures the stream itself
def test_zz_sequence_inside_a_callers_stream_capture():
    """lstm_seq_fwd + lstm_seq_bwd(use_graph=True) inside one torch.cuda.graph capture (a linear chain): the library must
    not replay a graph of its own into a capturing stream; it enqueues plain launches, which the caller's graph records.
    Two replays are bit-identical to plain launches; the library's counters do not move.  Kept last in this file."""
    ops = _ops()
    q_len, dirs = R.make_case(5, 64, 3, (False, True), True, True, seed=79)
    refs = [R.ref_of(q_len, d) for d in dirs]
    run = Run(q_len, dirs)
    run.fwd(False)                                # also the warm-up: kernel attributes are set outside the capture
    run.bwd(False)
    torch.cuda.synchronize()
    run.check(refs, "plain launches before the capture")
    plain = [run.got(k) for k in range(run.ndir)]
    run.reset()
    before = ops.lstm_graph_stats()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run.fwd(True)
        run.bwd(True)
    assert ops.lstm_graph_stats() == before, (before, ops.lstm_graph_stats())
    for rep in range(2):
        run.reset()
        g.replay()
        torch.cuda.synchronize()
        for k in range(run.ndir):
            got = run.got(k)
            for name, ref in plain[k].items():
                assert torch.equal(got[name].view(torch.int32), ref.view(torch.int32)), (rep, k, name)
        run.check_guards()
    assert ops.lstm_graph_stats() == before
