"""CPU: host-side argument validation of the two plain softmax + weighted-sum entry points, vqa_att_apply_fwd and
vqa_att_apply_bwd -- the checks their gather forms have (tests/test_multi_question_cpu.py, tests/test_shared_train_cpu.py).
Pointers are made-up 16-byte-aligned integers: every check runs on the host before any HIP call, nothing dereferences them."""


def _caller(f, names, ok):
    def call(**ch):
        a = list(ok)
        for k, val in ch.items():
            a[names.index(k)] = val
        return f(*a)
    return call


def test_apply_fwd_argument_validation_without_gpu():
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    names = ("score", "vn", "probs", "out", "out_ld", "B", "P", "C", "G", "stream")
    call = _caller(lib.vqa_att_apply_fwd, names, (16, 16, 16, 16, 64, 3, 4, 8, 2, None))
    for name in ("score", "vn", "probs", "out"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(G=0) == 1 and b"glimpses" in err()
    assert call(G=9) == 1 and b"glimpses" in err()
    assert call(G=9, P=20000) == 1 and b"glimpses" in err()        # before the LDS size is computed from G
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(B=-1) == 1 and b"out of range" in err()
    assert call(C=0) == 1 and b"out of range" in err()
    assert call(out_ld=8) == 1 and b"out_ld=8" in err()            # out_ld < G*C
    assert call(P=20000) == 1 and b"too large for LDS" in err()    # G*P floats of probabilities
    assert call(B=0) == 0                                          # no launch
    assert call(B=0, vn=20, C=6) == 0                              # odd width, unaligned vn: served (the scalar kernels)


def test_apply_bwd_argument_validation_without_gpu():
    from dl_vqa_amd import _lib
    lib = _lib.load()
    err = lib.vqa_last_error
    names = ("dout", "dout_ld", "probs", "vn", "dscore", "dvn", "rowsum", "B", "P", "C", "G", "stream")
    call = _caller(lib.vqa_att_apply_bwd, names, (16, 64, 16, 16, 16, 16, 16, 3, 4, 8, 2, None))
    for name in ("dout", "probs", "vn", "dscore"):
        assert call(**{name: None}) == 1 and b"null pointer" in err(), name
    assert call(G=0) == 1 and b"glimpses" in err()
    assert call(G=9) == 1 and b"glimpses" in err()
    assert call(P=0) == 1 and b"out of range" in err()
    assert call(B=-1) == 1 and b"out of range" in err()
    assert call(C=6) == 1 and b"C=6" in err()                      # C % 4
    assert call(C=0) == 1 and b"C=0" in err()
    assert call(dout_ld=8) == 1 and b"dout_ld=8" in err()          # dout_ld < G*C
    assert call(dout_ld=18) == 1 and b"dout_ld=18" in err()        # dout_ld % 4
    for name in ("dout", "vn", "dvn"):
        assert call(**{name: 20}) == 1 and b"aligned" in err(), name
    assert call(P=20000, B=0) == 0                                 # no LDS bound in the backward
    assert call(B=0) == 0                                          # no launch
    assert call(B=0, dvn=None, rowsum=None) == 0                   # both are optional (what the train step passes)
