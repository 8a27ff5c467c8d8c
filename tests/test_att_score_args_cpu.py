"""CPU: host-side argument validation of the two plain attention-score entry points, vqa_att_score_fwd and
vqa_att_score_bwd -- the checks their grouped forms have (tests/test_multi_question_cpu.py, tests/test_shared_train_cpu.py).
Pointers are made-up 16-byte-aligned integers: every check runs on the host before any HIP call, nothing dereferences them."""


def _caller(f, names, ok):
    def call(**ch):
        a = list(ok)
        for k, val in ch.items():
            a[names.index(k)] = val
        return f(*a)
    return call


def test_score_fwd_argument_validation_without_gpu():
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    names = ("xs", "xs_is_bf16", "wx", "wx_ld", "bx", "score", "B", "P", "mid", "G", "p", "seed", "qcat", "stream")
    call = _caller(lib.vqa_att_score_fwd, names, (16, 0, 16, 8, 16, 16, 3, 4, 8, 2, 0.3, 1, None, None))
    for name in ("xs", "wx", "bx", "score"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(G=0) == 1 and b"glimpses" in err()
    assert call(G=9) == 1 and b"glimpses" in err()
    assert call(B=-1) == 1 and b"out of range" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(mid=6) == 1 and b"mid=6" in err()                  # mid % 4
    assert call(mid=0) == 1 and b"mid=0" in err()
    assert call(wx_ld=6, mid=4) == 1 and b"wx_ld=6" in err()       # wx_ld % 4
    assert call(qcat=16) == 1 and b"wx_ld=8" in err()              # '|': wx_ld = 8 < 2 * mid
    assert call(p=1.0) == 1 and b"p=1" in err()
    assert call(p=-0.5) == 1 and b"p=-0.5" in err()
    assert call(wx=20) == 1 and b"aligned" in err()
    assert call(qcat=20, wx_ld=16) == 1 and b"aligned" in err()
    assert call(xs=20, B=0) == 0                                   # an unaligned xs is served (the general kernel)
    assert call(B=0) == 0                                          # no launch
    assert call(B=0, qcat=16, wx_ld=16) == 0


def test_score_bwd_argument_validation_without_gpu():
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    names = ("dscore", "wx", "wx_ld", "xs", "xs_is_bf16", "dwx_part", "dq_part", "B", "P", "mid", "G", "p", "seed", "mode",
             "vprime", "qp", "stream")
    call = _caller(lib.vqa_att_score_bwd, names, (16, 16, 8, 16, 0, 16, 16, 3, 4, 8, 2, 0.3, 1, 0, None, None, None))
    for name in ("dscore", "wx", "xs", "dwx_part", "dq_part"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(G=0) == 1 and b"glimpses" in err()
    assert call(G=9) == 1 and b"glimpses" in err()
    assert call(B=-1) == 1 and b"out of range" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(mid=6) == 1 and b"mid=6" in err()
    assert call(mid=0) == 1 and b"mid=0" in err()
    assert call(wx_ld=6, mid=4) == 1 and b"wx_ld=6" in err()
    assert call(p=1.0) == 1 and b"p=1" in err()
    assert call(p=-0.5) == 1 and b"p=-0.5" in err()
    assert call(mode=3) == 1 and b"mode 3" in err()
    assert call(mode=1, qp=16) == 1 and b"null pointer" in err()                   # '*' reads v' ...
    assert call(mode=1, vprime=16) == 1 and b"null pointer" in err()               # ... and q'
    assert call(mode=2, wx_ld=16) == 1 and b"null pointer" in err()                # '|' reads q'
    assert call(mode=2, qp=16) == 1 and b"wx_ld=8" in err()                        # '|': wx_ld = 8 < 2 * mid
    for name in ("wx", "dwx_part", "dq_part"):
        assert call(**{name: 20}) == 1 and b"aligned" in err(), name
    assert call(mode=1, vprime=20, qp=16) == 1 and b"aligned" in err()
    assert call(mode=2, qp=20, wx_ld=16) == 1 and b"aligned" in err()
    assert call(B=0) == 0                                          # no launch (the grid (B, RS) would be invalid)
    assert call(B=0, mode=1, vprime=16, qp=16) == 0
    assert call(B=0, mode=2, qp=16, wx_ld=16) == 0
    assert call(B=0, xs=20) == 0                                   # xs is not among the checked quads
