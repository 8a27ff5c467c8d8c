"""Float64 reference of the masked LSTM recurrence of one direction, forward and explicit BPTT (CPU, no HIP).

The operation is what csrc/lstm.hip computes per direction (vqa_lstm_seq_fwd / vqa_lstm_seq_bwd): gate order i, f, g, o;
sample b advances at time t iff t < q_len[b] (the packed-sequence rule), otherwise its state is carried over unchanged;
the reverse direction visits t = T-1 .. 0.  State chains follow the library's slot convention: at time t the forward
direction reads slot t and writes slot t+1 of Hs / Cs [T+1,B,H], the reverse direction reads slot t+1 and writes slot t.

The backward pass is written out (no autograd), so every intermediate the kernels store or leave behind has a value here.
tests/test_lstm_ref_cpu.py ties all of it to torch.nn.LSTM.
"""
import torch

MUTANTS = ("le", "swap_slots", "no_passthrough")


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max|got - ref| / max|ref| in float64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def time_order(T: int, reverse: bool):
    """times in the order the forward pass visits them"""
    return list(range(T - 1, -1, -1)) if reverse else list(range(T))


def slots(t: int, reverse: bool):
    """(state slot read, state slot written) at time t"""
    return (t + 1, t) if reverse else (t, t + 1)


def lstm_dir_ref(xg, w_hh, q_len, reverse, h0=None, c0=None, dh_n=None, dc_n=None, mutant=None, dtype=torch.float64):
    """One direction.  xg [T,B,4H] gate pre-activation input (x W_ih^T + biases), w_hh [4H,H], q_len [B] integers,
    (h0, c0) [B,H] initial state, (dh_n, dc_n) [B,H] = d loss / d (h_n, c_n); None = zeros.

    Returns a dict of `dtype` tensors:
      gates  [T,B,4H]   activated gates, zero rows where (t, b) is inactive
      Hs, Cs [T+1,B,H]  state chains in the slot convention (initial slot = (h0, c0))
      h_n, c_n [B,H]    final state
      dgates [T,B,4H]   d loss / d gate pre-activations, zero rows where inactive
      dh_first [B,H]    d loss / d h at the first processed time: the total gradient w.r.t. the state that the first
                        visited time wrote (what BPTT holds in dh when it differentiates that time's cell)
      dh0, dc0 [B,H]    d loss / d h0, d loss / d c0
      active [T,B]      bool, t < q_len[b]

    mutant (tests only): a deliberately wrong neighbour of the rule -- "le": t <= q_len[b]; "swap_slots": the reverse
    direction reads slot t and writes slot t+1; "no_passthrough": the incoming dh of a finished sample is dropped instead
    of carried to the previous time."""
    assert mutant is None or mutant in MUTANTS
    T, B, H4 = xg.shape
    H = H4 // 4
    xg, w = xg.detach().cpu().to(dtype), w_hh.detach().cpu().to(dtype)
    ql = q_len.detach().cpu().to(torch.int64)
    z = lambda t_: torch.zeros(B, H, dtype=dtype) if t_ is None else t_.detach().cpu().to(dtype).clone()
    h0, c0, dh, dc = z(h0), z(c0), z(dh_n), z(dc_n)
    order = time_order(T, reverse)

    def sl(t):
        si, so = slots(t, reverse)
        return (so, si) if (mutant == "swap_slots" and reverse) else (si, so)

    Hs, Cs = torch.zeros(T + 1, B, H, dtype=dtype), torch.zeros(T + 1, B, H, dtype=dtype)
    gates = torch.zeros(T, B, 4 * H, dtype=dtype)
    active = torch.zeros(T, B, dtype=torch.bool)
    init = T if reverse else 0
    Hs[init], Cs[init] = h0, c0
    for t in order:
        si, so = sl(t)
        h, c = Hs[si], Cs[si]
        i, f, g, o = (xg[t] + h @ w.t()).split(H, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        act = (t <= ql) if mutant == "le" else (t < ql)
        a = act.unsqueeze(1)
        cn = f * c + i * g
        hn = o * torch.tanh(cn)
        gates[t] = torch.where(a, torch.cat([i, f, g, o], dim=1), torch.zeros((), dtype=dtype))
        Cs[so] = torch.where(a, cn, c)
        Hs[so] = torch.where(a, hn, h)
        active[t] = act
    last = sl(order[-1])[1]
    h_n, c_n = Hs[last].clone(), Cs[last].clone()

    dgates = torch.zeros(T, B, 4 * H, dtype=dtype)
    dh_first = None
    for t in reversed(order):
        si, so = sl(t)
        a = active[t].unsqueeze(1)
        gi, gf, gg, go = gates[t].split(H, dim=1)
        tc = torch.tanh(Cs[so])
        dct = dc + dh * go * (1 - tc * tc)
        dg = torch.cat([dct * gg * gi * (1 - gi), dct * Cs[si] * gf * (1 - gf), dct * gi * (1 - gg * gg),
                        dh * tc * go * (1 - go)], dim=1)
        dgates[t] = torch.where(a, dg, torch.zeros((), dtype=dtype))
        dc = torch.where(a, dct * gf, dc)
        if t == order[0]:
            dh_first = dh.clone()
        carried = torch.zeros_like(dh) if mutant == "no_passthrough" else dh
        dh = dgates[t] @ w + torch.where(a, torch.zeros((), dtype=dtype), carried)
    return dict(gates=gates, Hs=Hs, Cs=Cs, h_n=h_n, c_n=c_n, dgates=dgates, dh_first=dh_first, dh0=dh, dc0=dc,
                active=active)


def ragged_lengths(B: int, T: int, g: torch.Generator) -> torch.Tensor:
    """lengths in [1, T] that include T (first sample) and 1 (last sample; B == 1: T only)"""
    q_len = torch.randint(1, T + 1, (B,), generator=g)
    q_len[-1] = 1
    q_len[0] = T
    return q_len


def make_case(B, H, T, ndir_rev, state, dh_in, seed):
    """Inputs of one test case, float32 on the CPU.  ndir_rev: tuple of `reverse` flags, one per direction; state / dh_in:
    non-zero (randn * 0.5) initial state / incoming dh, else zeros.  Returns (q_len, [per-direction dict])."""
    g = torch.Generator().manual_seed(seed)
    q_len = ragged_lengths(B, T, g)
    rn = lambda *s, k=1.0: torch.randn(*s, generator=g) * k
    dirs = []
    for rev in ndir_rev:
        d = dict(reverse=bool(rev), w_hh=rn(4 * H, H) / H ** 0.5, xg=rn(T, B, 4 * H), dc_n=rn(B, H))
        d["h0"], d["c0"] = (rn(B, H, k=0.5), rn(B, H, k=0.5)) if state else (torch.zeros(B, H), torch.zeros(B, H))
        d["dh_n"] = rn(B, H) if dh_in else torch.zeros(B, H)
        dirs.append(d)
    return q_len, dirs


# The GPU test's cases: (B, H, T, reverse flag per direction, non-zero initial state, non-zero incoming dh).  The smallest
# shapes at which the kernels can go wrong: forward tile 64 rows x 16 units x 4 gates, backward tile 64 x 32 over K = 4H,
# K-step 32 with a two-stage ring -- B in {1, 63, 64, 65, 130}, H in {32 (one K-step), 64, 96 (odd step count), 160 (five
# backward column tiles)}, T in {1, 2, 14, 30}, a single direction that is the reverse one, and grids that are no
# multiple of 8 workgroups (forward / backward workgroups per launch in the comments).
F, R = False, True
CASES = [
    (1, 32, 1, (F,), True, True),          # 2 / -   (T = 1: the first-step kernel alone)
    (1, 32, 2, (R,), False, True),         # 2 / 1
    (63, 64, 14, (F, R), True, False),     # 8 / 4
    (64, 96, 2, (R,), True, True),         # 6 / 3
    (65, 32, 14, (F, R), False, True),     # 8 / 4
    (65, 96, 30, (F,), True, False),       # 12 / 6
    (130, 160, 30, (F, R), True, True),    # 60 / 30
    (130, 64, 1, (F, R), False, False),    # 24 / -
    (64, 160, 14, (R,), False, False),     # 10 / 5
    (63, 32, 30, (R,), True, True),        # 2 / 1
    (1, 160, 14, (F, R), False, True),     # 20 / 10
    (64, 64, 2, (F,), False, False),       # 4 / 2
]


def case_inputs(idx: int):
    B, H, T, revs, state, dh_in = CASES[idx]
    return make_case(B, H, T, revs, state, dh_in, seed=1000 + idx)


def ref_of(q_len, d, mutant=None, dtype=torch.float64):
    return lstm_dir_ref(d["xg"], d["w_hh"], q_len, d["reverse"], d["h0"], d["c0"], d["dh_n"], d["dc_n"], mutant=mutant,
                        dtype=dtype)


# what the GPU test compares, and at which of the project's two bounds (max|err| / max|ref|)
FWD_TOL, BWD_TOL = 5e-6, 2e-5
COMPARED = (("gates", FWD_TOL), ("Hs", FWD_TOL), ("Cs", FWD_TOL), ("c_n", FWD_TOL), ("dgates", BWD_TOL),
            ("dh_first", BWD_TOL), ("dc0", BWD_TOL))


def tol_for(base: float, T: int) -> float:
    """The bound at T steps: the per-step activation error (<= 3e-7 absolute, csrc/lstm.hip) adds as a random walk, so the
    T <= 5 bound is scaled by sqrt(T / 5) beyond that."""
    return base * max(1.0, (T / 5.0) ** 0.5)


def compare(got: dict, ref: dict, T: int, label: str = "", emit=print):
    """The GPU test's parity comparison: every output in COMPARED (that `got` holds: a forward-only result has no
    gradients) against the reference at its bound.  Returns the names that exceed their bound (an empty list = pass) and
    prints one [parity] line per output."""
    bad = []
    for name, base in COMPARED:
        if name not in got:
            continue
        tol = tol_for(base, T)
        g = got[name]
        e = rel_err(g, ref[name]) if bool(torch.isfinite(g).all()) else float("inf")
        if emit is not None:
            emit(f"[parity] lstm {label} {name}: max|err|/max|ref| = {e:.3e} (tol {tol:.2e})")
        if not e <= tol:
            bad.append(name)
    return bad


def exact_violations(got: dict, active: torch.Tensor, reverse: bool):
    """The GPU test's exact checks on a result in the slot convention: gate and dgates rows of an inactive (t, b) are 0.0,
    and the state written for an inactive (t, b) has the bits of the slot it was read from.  Returns a list of messages."""
    T = active.shape[0]
    bad = []
    for t in range(T):
        idle = ~active[t]
        if not bool(idle.any()):
            continue
        si, so = slots(t, reverse)
        for name in ("gates", "dgates"):
            if name not in got:
                continue
            rows = got[name][t][idle]
            if not torch.equal(rows, torch.zeros_like(rows)):
                bad.append(f"{name}[{t}] has a non-zero inactive row")
        for name in ("Hs", "Cs"):
            a, b = got[name][so][idle], got[name][si][idle]
            if not torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                               b.view(torch.int64 if b.dtype == torch.float64 else torch.int32)):
                bad.append(f"{name}: slot {so} of a sample inactive at t={t} differs from slot {si}")
    return bad
