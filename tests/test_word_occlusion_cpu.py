"""CPU: exact word occlusion from cached features (VqaNet.explain_words_occlusion) -- the host variant table, the prefix claim
in float64 (chains that start from the base run's saved states give what a full forward per variant gives), the scale of the
signal and its distance from the gradient x input words, the two new entry points' host-side argument validation, and the
errors the public call raises before any device work, which are explain_words' (those every explain call shares:
tests/test_explain_refusals_cpu.py)."""
import pytest
import torch

from dl_vqa_amd import WordOcclusion
from dl_vqa_amd.model import word_occlusion_chunks, word_occlusion_table
from tests import attribution_ref as R
from tests import word_occlusion_ref as WO
from tests.explain_util import host_caches, tiny as _tiny


# ----------------------------------------------------------------------------- the host table
def _check_table(lengths, T, b0=0, b1=None):
    B = len(lengths)
    b1 = B if b1 is None else b1
    tab = word_occlusion_table(lengths, T, b0, b1)
    want = [(t, b) for b in range(b0, b1) for t in range(min(max(lengths[b], 0), T))]
    assert tab.V == len(want) == sum(min(max(n, 0), T) for n in lengths[b0:b1])
    fwd = list(zip(tab.fwd_t.tolist(), tab.fwd_b.tolist()))
    rev = list(zip(tab.rev_t.tolist(), tab.rev_b.tolist()))
    assert fwd == sorted(want)                                               # ascending t: the order the forward chains start in
    assert rev == sorted(want, key=lambda p: (-p[0], p[1]))                  # descending t: the reverse chains'
    assert [fwd[r] for r in tab.rev_row.tolist()] == rev
    assert tab.fwd_seed.tolist() == [t * B + b for t, b in fwd] and tab.rev_seed.tolist() == [(t + 1) * B + b for t, b in rev]
    for dtype_of in (tab.fwd_b, tab.fwd_t, tab.fwd_seed, tab.rev_b, tab.rev_t, tab.rev_seed, tab.rev_row):
        assert dtype_of.dtype == torch.int32 and not dtype_of.is_cuda
    assert len(tab.n_fwd) == len(tab.n_rev) == T
    for s in range(T):
        assert tab.n_fwd[s] == sum(1 for t, _ in want if t <= s)             # the rows whose chain has started at time s ...
        assert tab.n_rev[s] == sum(1 for t, _ in want if t >= s)
        assert all(t <= s for t, _ in fwd[:tab.n_fwd[s]]) and all(t > s for t, _ in fwd[tab.n_fwd[s]:])    # ... are the first n_s
        assert all(t >= s for t, _ in rev[:tab.n_rev[s]]) and all(t < s for t, _ in rev[tab.n_rev[s]:])
    assert tab.steps == max([min(max(n, 0), T) for n in lengths[b0:b1]], default=0)
    assert tab.row_steps == sum(tab.n_fwd[:tab.steps]) + sum(tab.n_rev[:tab.steps])
    assert tab.row_steps <= tab.V * (T + 1) and all(n == 0 for n in tab.n_rev[tab.steps:])
    if tab.V:
        assert tab.row_steps < 2 * T * tab.V or T == 1
    return tab


@pytest.mark.parametrize("lengths,T", [((5, 3, 1, 5, 3, 1, 3), 5), ((6, 1, 4, 6, 3), 6), ((6, 1, 4, 6, 3), 1)])
def test_host_table(lengths, T):
    lengths = list(lengths)
    tab = _check_table(lengths, T)
    assert tab.V == sum(min(n, T) for n in lengths)
    # lengths 0, negative and above T: no variant, resp. T of them
    odd = [0, T + 3, 2, -1, T]
    tab = _check_table(odd, T)
    assert tab.V == T + min(2, T) + T and 0 not in tab.fwd_b.tolist() and 3 not in tab.fwd_b.tolist()
    assert _check_table([0, 0], T).V == 0 and _check_table([], T).V == 0
    # a tensor of lengths gives what the list gives
    again = word_occlusion_table(torch.tensor(lengths), T)
    assert again.fwd_b.tolist() == _check_table(lengths, T).fwd_b.tolist() and again.n_rev == _check_table(lengths, T).n_rev


@pytest.mark.parametrize("lengths,T", [((5, 3, 1, 5, 3, 1, 3), 5), ((6, 1, 4, 6, 3), 6), ((6, 1, 4, 6, 3), 1), ((0, 9, 2, 0), 5)])
def test_chunks_cut_between_questions(lengths, T):
    lengths = list(lengths)
    B = len(lengths)
    assert word_occlusion_chunks(lengths, T) == [(0, B)] and word_occlusion_chunks([], T, 4) == []
    total = _check_table(lengths, T).V
    for cap in (1, 2, 3, 6, 7, 100):
        chunks = word_occlusion_chunks(lengths, T, cap)
        assert chunks[0][0] == 0 and chunks[-1][1] == B
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(b0 < b1 for b0, b1 in chunks)
        seen = []
        for b0, b1 in chunks:
            tab = _check_table(lengths, T, b0, b1)
            assert tab.V <= cap or b1 - b0 == 1 or all(min(max(n, 0), T) == 0 for n in lengths[b0 + 1:b1])
            assert set(tab.fwd_b.tolist()) <= set(range(b0, b1))             # a question's variants are all in its chunk
            seen += list(zip(tab.fwd_b.tolist(), tab.fwd_t.tolist()))
        assert len(seen) == total == len(set(seen))
    assert len(word_occlusion_chunks(lengths, T, 1)) >= sum(1 for n in lengths if n > 0)


# ----------------------------------------------------------------------------- the prefix claim, in float64
def _fixture_args(do_option):
    f = R.fixture_case(do_option)
    return f, (f["golden"].sd, do_option, f["vn"], f["q"], f["q_len"], f["img"])


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_prefix_shared_chains_equal_the_brute_force(do_option):
    f, args = _fixture_args(do_option)
    B, T = f["q"].shape
    A, bidir = f["cfg"]["max_answers"], f["cfg"]["text"]["bidirectional"]
    top = R.forward64(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], f["grid"]).argmax(1).tolist()
    V = len(WO.variants(f["q_len"], T))
    for cols in (top, WO.columns(B, A)):
        want = WO.fixture_brute(do_option, cols)
        for rows in (None, 3):
            got, row_steps = WO.prefix_shared(*args, cols, f["grid"], bidir, chunk_rows=rows)
            err = float((got - want).abs().max())
            print(f"[identity-word-occlusion] {R.FIXTURES[do_option]} chunk rows {rows}: prefix-shared vs brute force {err:.3e}, "
                  f"max|words| {float(want.abs().max()):.3e}; row-steps {row_steps} of {2 * T * V} ({V} variants, T = {T})")
            assert err < 1e-12
            assert row_steps <= V * (T + 1) < 2 * T * V
    pad = torch.arange(T)[None, :] >= f["q_len"][:, None]
    assert bool(pad.any()) and bool((want[pad] == 0).all())


@pytest.mark.parametrize("bidirectional", [True, False])
def test_prefix_shared_chains_on_the_random_cases(bidirectional):
    from tests import word_attribution_ref as W
    for T in (6, 1):
        case = W.random_case(bidirectional, T)
        B = case["q"].shape[0]
        cols = WO.columns(B, case["cfg"]["max_answers"])
        want = WO.case_brute(case, "+", cols)
        got, _ = WO.prefix_shared(case["sd"], "+", case["vn"], case["q"], case["q_len"], case["img"], cols, case["grid"],
                                  bidirectional)
        assert float(want.abs().max()) > 0 and float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("do_option", ["+", "*", "|"])
def test_scale_of_the_signal_and_distance_from_gradient_x_input(do_option):
    """A test on `words` cannot pass with zeros or with explain_words' first-order values."""
    f, _ = _fixture_args(do_option)
    top = R.forward64(f["golden"].sd, do_option, f["vn"], f["qf"], f["img"], f["grid"]).argmax(1).tolist()
    exact = WO.fixture_brute(do_option, top)
    estimate = WO.first_order(f, do_option, top)
    peak = float(exact.abs().max())
    gap = float((exact - estimate).abs().max()) / peak
    print(f"[identity-word-occlusion] {R.FIXTURES[do_option]}: max|words| = {peak:.3e}, |occlusion - gradient x input| = {gap:.3f} "
          f"of it")
    assert peak > 1e-2 and gap > 0.30


def test_a_zero_embedding_row_gives_zero_by_definition_in_float64():
    """Token 0 (a zero row) inside a question: the definition gives exactly 0 there -- the device's few ulp are two kernel
    routes' difference, not a property of the quantity."""
    f, _ = _fixture_args("+")
    sd = f["golden"].sd
    assert float(sd["text.embedding.weight"][0].abs().max()) == 0.0
    q = f["q"].clone()
    q[0, 0] = 0
    words, _ = WO.brute(sd, "+", f["vn"], q, f["q_len"], f["img"], [0] * len(q), f["grid"], f["cfg"]["text"]["bidirectional"])
    assert float(words[0, 0]) == 0.0 and float(words[0].abs().max()) > 0


# ----------------------------------------------------------------------------- the ABI: host-side argument validation
def test_entry_points_are_declared_bound_and_wrapped():
    from dl_vqa_amd import _lib, build, ops
    build.build_library(verbose=False)
    lib = _lib.load()
    assert lib.vqa_abi_version() == _lib.header_abi_version() == 9           # appended, not bumped
    for name in ("vqa_lstm_occl_cell_fwd", "vqa_occl_words"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert list(_lib.PROTOTYPES)[-2:] == ["vqa_gather_rows_drop_norm", "vqa_gather_rows_drop_norm_f16"]
    assert callable(ops.lstm_occl_cell_fwd) and callable(ops.occl_words)


def test_lstm_occl_cell_argument_validation_without_gpu():
    """Pointers are made-up aligned integers: every check runs on the host before any HIP call, and n == 0 launches nothing."""
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err, f = lib.vqa_last_error, lib.vqa_lstm_occl_cell_fwd
    ok = dict(xg_base=16, xg0=16, hg=16, h_var=16, c_var=16, st_ld=8, q_len=16, var_b=16, var_t=16, s=1, c_final=16, cf_ld=24,
              cf_row=16, n=0, B=3, T=4, H=8, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    assert call() == 0 and call(c_final=None, cf_row=None, cf_ld=0) == 0
    for name in ("xg_base", "xg0", "hg", "h_var", "c_var", "q_len", "var_b", "var_t"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    for bad in (dict(n=-1), dict(B=0), dict(T=0), dict(H=0), dict(s=-1), dict(s=4)):
        assert call(**bad) == 1 and b"out of range" in err(), bad
    assert call(st_ld=7) == 1 and b"row stride" in err()
    assert call(cf_ld=7) == 1 and b"c_final" in err()
    assert call(c_final=None) == 1 and b"cf_row without c_final" in err()


def test_occl_words_argument_validation_without_gpu():
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err, f = lib.vqa_last_error, lib.vqa_occl_words
    ok = dict(h1=16, h1_ld=8, W2=16, w2_ld=8, b2=16, answers=16, logits=16, logits_ld=5, var_b=16, var_t=16, q_len=16, words=16, n=3,
              b0=0, nb=0, T=4, hid=8, A=5, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    assert call(n=0) == 0 and call(n=0, h1=None, var_b=None, var_t=None) == 0       # no questions: nothing launched
    for name in ("W2", "b2", "answers", "logits", "q_len", "words"):
        assert call(**{name: None}, n=0) == 1 and b"null pointer" in err(), name
    for name in ("h1", "var_b", "var_t"):
        assert call(**{name: None}, nb=1) == 1 and b"null pointer" in err(), name
    for bad in (dict(n=-1), dict(b0=-1), dict(nb=-1), dict(T=0), dict(hid=0), dict(A=0)):
        assert call(**bad) == 1 and b"out of range" in err(), bad
    assert call(n=3, nb=0) == 1 and b"variant rows" in err()                         # more rows than the questions have slots
    assert call(n=5, nb=1) == 1 and b"variant rows" in err()
    for bad in (dict(h1_ld=7), dict(w2_ld=7), dict(logits_ld=4)):
        assert call(**bad, n=0) == 1 and b"out of range" in err(), bad


# ----------------------------------------------------------------------------- errors before any device work
def _host_features(m, N=3, vprime=True):
    return host_caches(m, N, vprime=vprime)[0]


# (what the six explain calls refuse alike: tests/test_explain_refusals_cpu.py)
def test_refusals_that_need_no_device():
    assert WordOcclusion._fields == ("words", "answers", "logits")
    g, m = _tiny()
    m.eval()
    A = m._engine.A
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    feats = _host_features(m)
    # what explain_words raises for the same arguments, the call's own name in the message
    _, other = _tiny()
    other.eval()
    theirs = _host_features(other)

    def raised(run):
        with pytest.raises(Exception) as e:
            run()
        return type(e.value), str(e.value).replace("explain_words_occlusion", "explain_words")

    for images in (feats, theirs, _host_features(m, vprime=False)):
        for index in ([0, 1, 2], [0, 1, feats.N], [0, 1]):
            for answers in (None, [0, 1], [0, A - 1, 1]):
                assert raised(lambda: m.explain_words_occlusion(images, q, ql, index, answers=answers)) == \
                    raised(lambda: m.explain_words(images, q, ql, index, answers=answers))
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())
