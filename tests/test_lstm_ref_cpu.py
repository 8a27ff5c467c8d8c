"""tests/lstm_ref.py against torch.nn.LSTM, and the GPU test's comparison against three wrong neighbours of the rule.

nn.LSTM(input_size=4H, hidden_size=H, bidirectional=True).double() with weight_ih = I and zero biases takes the gate
pre-activation input itself as x, so x.grad of a loss on one direction's (h_n, c_n) is that direction's dgates.  It is fed
through pack_padded_sequence(enforce_sorted=False) with a non-zero (h0, c0); every output of the reference must agree to
1e-12 in both directions.  nn.LSTM shows h per step and the final state only, so the per-step cell states come from runs on
prefixes (forward direction) and suffixes (reverse direction) of the same sequence, the gate activations from the
nn.LSTM-verified h chain, and d loss / d h at the first processed time from a run that starts behind that time.
"""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from tests import lstm_ref as R

TOL = 1e-12


def _nn_lstm(H, w):
    m = torch.nn.LSTM(input_size=4 * H, hidden_size=H, bidirectional=True).double()
    with torch.no_grad():
        for sfx, wd in (("", w[0]), ("_reverse", w[1])):
            getattr(m, "weight_ih_l0" + sfx).copy_(torch.eye(4 * H, dtype=torch.float64))
            getattr(m, "weight_hh_l0" + sfx).copy_(wd)
            getattr(m, "bias_ih_l0" + sfx).zero_()
            getattr(m, "bias_hh_l0" + sfx).zero_()
    return m


def _run(m, x, lens, h0, c0):
    """(padded outputs [T',B,2H], h_n [2,B,H], c_n [2,B,H]) of the packed run"""
    out, (hn, cn) = m(pack_padded_sequence(x, lens, enforce_sorted=False), (h0, c0))
    return pad_packed_sequence(out, total_length=x.shape[0])[0], hn, cn


def _close(name, got, ref):
    e = float((got - ref).abs().max())
    print(f"[parity] lstm_ref vs nn.LSTM {name}: max abs err {e:.3e}")
    assert e <= TOL, (name, e)


@pytest.mark.parametrize("B,H,T", [(5, 32, 14), (7, 32, 30), (3, 32, 1)])
def test_reference_matches_nn_lstm_in_both_directions(B, H, T):
    g = torch.Generator().manual_seed(B * 100 + T)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q_len = R.ragged_lengths(B, T, g)
    w = [rn(4 * H, H) / H ** 0.5 for _ in range(2)]
    xg = rn(T, B, 4 * H)
    h0, c0, dhn, dcn = (rn(2, B, H) * 0.5 for _ in range(4))
    m = _nn_lstm(H, w)
    x = xg.clone().requires_grad_(True)
    h0r, c0r = h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    out, hn, cn = _run(m, x, q_len, h0r, c0r)
    for d, rev in enumerate((False, True)):
        ref = R.lstm_dir_ref(xg, w[d], q_len, rev, h0[d], c0[d], dhn[d], dcn[d])
        tag = "rev" if rev else "fwd"
        act = ref["active"]
        assert torch.equal(act, torch.arange(T)[:, None] < q_len[None, :])
        # ---- final state and the gradients of a loss on this direction alone
        gx, gh, gc = torch.autograd.grad((hn[d] * dhn[d]).sum() + (cn[d] * dcn[d]).sum(), (x, h0r, c0r), retain_graph=True)
        _close(f"{tag} h_n", ref["h_n"], hn[d].detach())
        _close(f"{tag} c_n", ref["c_n"], cn[d].detach())
        _close(f"{tag} dgates", ref["dgates"], gx)
        _close(f"{tag} dh0", ref["dh0"], gh[d])
        _close(f"{tag} dc0", ref["dc0"], gc[d])
        assert float(gh[1 - d].abs().max()) == 0.0
        # ---- the h chain from the padded outputs: an active (t, b) wrote out[t, b]; an inactive one carried its slot over
        Hs = torch.empty(T + 1, B, H, dtype=torch.float64)
        Hs[T if rev else 0] = h0[d]
        o = out.detach()[:, :, d * H:(d + 1) * H]
        for t in R.time_order(T, rev):
            si, so = R.slots(t, rev)
            Hs[so] = torch.where(act[t][:, None], o[t], Hs[si])
        _close(f"{tag} Hs", ref["Hs"], Hs)
        # ---- the c chain: c_n of the run that stops after time t (forward: prefix, lengths cut at t + 1; reverse: the suffix
        # from t on, lengths q_len - t, for the samples that have reached it; the others still hold c0)
        Cs = torch.empty(T + 1, B, H, dtype=torch.float64)
        Cs[T if rev else 0] = c0[d]
        with torch.no_grad():
            for t in range(T):
                if rev:
                    on = q_len > t
                    Cs[t] = c0[d]
                    Cs[t][on] = _run(m, xg[t:, on], q_len[on] - t, h0[:, on].contiguous(), c0[:, on].contiguous())[2][1]
                else:
                    Cs[t + 1] = _run(m, xg[:t + 1], q_len.clamp(max=t + 1), h0, c0)[2][0]
        _close(f"{tag} Cs", ref["Cs"], Cs)
        # ---- gate activations from the verified h chain, zero rows where inactive
        gates = torch.zeros(T, B, 4 * H, dtype=torch.float64)
        for t in range(T):
            i, f, gg, oo = (xg[t] + Hs[R.slots(t, rev)[0]] @ w[d].t()).split(H, dim=1)
            gates[t] = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(oo)], dim=1) * act[t][:, None]
        _close(f"{tag} gates", ref["gates"], gates)
        # ---- d loss / d h at the first processed time t0: a sample inactive there carried h0 through it, so it is dh0; a
        # sample whose only step is t0 gets dh_n itself; the others get the h0 gradient of the run that starts behind t0
        t0 = R.time_order(T, rev)[0]
        exp = gh[d].clone()
        more = act[t0] & (q_len > 1)
        only = act[t0] & (q_len == 1)
        exp[only] = dhn[d][only]
        if bool(more.any()):
            s0 = R.slots(t0, rev)[1]
            hs = torch.zeros(2, int(more.sum()), H, dtype=torch.float64)
            cs = torch.zeros_like(hs)
            hs[d], cs[d] = Hs[s0][more], Cs[s0][more]
            hs.requires_grad_(True)
            xs = xg[:T - 1, more] if rev else xg[1:, more]
            _, hn2, cn2 = _run(m, xs, q_len[more] - 1, hs, cs)
            exp[more] = torch.autograd.grad((hn2[d] * dhn[d][more]).sum() + (cn2[d] * dcn[d][more]).sum(), hs)[0][d]
        _close(f"{tag} dh_first", ref["dh_first"], exp)


def _distinguishable(mutant, q_len, T, d):
    """Does the mutant change an output that the GPU test compares, on these inputs?"""
    if mutant == "le":
        return bool((q_len < T).any())            # a sample of length L < T would also advance at t = L
    if mutant == "swap_slots":
        return d["reverse"]
    # no_passthrough: a forward-direction sample that finished early carries the incoming dh_n back to its last step (dgates);
    # a reverse-direction sample of length <= T - 2 carries its gradient through the times behind it into dh_first
    if d["reverse"]:
        return bool((q_len <= T - 2).any())
    return bool((q_len < T).any()) and float(d["dh_n"].abs().max()) > 0


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_gpu_comparison_rejects_the_rules_neighbours(mutant):
    """On the GPU test's own inputs the comparison it makes (float64 parity at its bounds + the exact checks) accepts a
    plain float32 evaluation of the rule and rejects each mutant wherever the mutant differs from the rule at all."""
    caught = 0
    for idx, (B, H, T, revs, state, dh_in) in enumerate(R.CASES):
        q_len, dirs = R.case_inputs(idx)
        assert int(q_len.max()) == T and (B == 1 or int(q_len.min()) == 1)
        for d in dirs:
            ref = R.ref_of(q_len, d)
            f32 = R.ref_of(q_len, d, dtype=torch.float32)
            assert R.compare(f32, ref, T, emit=None) == [] and R.exact_violations(f32, ref["active"], d["reverse"]) == []
            bad = R.ref_of(q_len, d, mutant=mutant)
            failed = R.compare(bad, ref, T, emit=None) or R.exact_violations(bad, ref["active"], d["reverse"])
            if _distinguishable(mutant, q_len, T, d):
                assert failed, (mutant, R.CASES[idx], d["reverse"])
                caught += 1
            else:
                assert not failed, (mutant, R.CASES[idx], d["reverse"])
    assert caught >= 4, (mutant, caught)


def test_cases_cover_the_edges():
    Bs, Hs, Ts, dirsets = (set(c[i] for c in R.CASES) for i in range(4))
    assert Bs == {1, 63, 64, 65, 130} and Hs == {32, 64, 96, 160} and Ts == {1, 2, 14, 30}
    assert dirsets == {(False,), (True,), (False, True)}
    assert (130, 160, 30, (False, True)) in [c[:4] for c in R.CASES]
    assert sum(c[4] for c in R.CASES) * 2 == len(R.CASES) and sum(c[5] for c in R.CASES) * 2 >= len(R.CASES)
    fwd_wg = [len(c[3]) * ((c[0] + 63) // 64) * (c[1] // 16) for c in R.CASES]
    bwd_wg = [len(c[3]) * ((c[0] + 63) // 64) * (c[1] // 32) for c in R.CASES if c[2] > 1]
    assert any(n % 8 for n in fwd_wg) and any(n % 8 for n in bwd_wg) and 2 in fwd_wg and 1 in bwd_wg
