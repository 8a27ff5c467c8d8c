"""CPU: what only VqaNet.explain_faithfulness_probs / explain_faithfulness_probs_pairs assert about their refusals: the maps
argument (explain_faithfulness' own check, in this call's name), and that every refusal is explain_faithfulness' refusal under
the other name.  What the whole explain family refuses is in tests/test_explain_refusals_cpu.py, these two calls included."""
import pytest
import torch

from dl_vqa_amd import ImageFeatures
from tests.explain_util import host_caches, tiny

# name, pairs form, the name of the logit call whose refusals these calls share
CALLS = [("explain_faithfulness_probs", False, "explain_faithfulness"),
         ("explain_faithfulness_probs_pairs", True, "explain_faithfulness_pairs")]
IDS = [call[0] for call in CALLS]
GOOD = torch.zeros(3, 2, 2)


def invoke(m, name, pairs, feats, qfeats, q, ql, index, maps=GOOD, **kw):
    """One call about three questions on host caches: the pairs forms ask the questions [0, 1, 1] of qfeats."""
    if pairs:
        return getattr(m, name)(feats, qfeats, index, [0, 1, 1], maps, **kw)
    return getattr(m, name)(feats, q, ql, index, maps, **kw)


@pytest.mark.parametrize("name,pairs,logit_name", CALLS, ids=IDS)
def test_the_maps_are_judged_on_the_host_before_answers_and_index(name, pairs, logit_name):
    g, m = tiny()
    m.eval()
    A = m._engine.A
    feats, qfeats = host_caches(m, N=3, M=2)                        # a 2 x 2 grid: P = 4
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    call = lambda maps=GOOD, index=(0, 1, 2), **kw: invoke(m, name, pairs, feats, qfeats, q, ql, list(index), maps, **kw)
    for bad in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 2, 2, dtype=torch.bool), [[1, 2, 3, 4]] * 3):
        with pytest.raises(TypeError, match=f"VqaNet.{name}: maps must be a floating tensor"):
            call(bad)
    for bad in (torch.zeros(3, 5), torch.zeros(2, 2, 2), torch.zeros(12), torch.zeros(4, 3), torch.zeros(3, 4, 1),
                torch.zeros(3, 1, 4), torch.zeros(3, 2, 2, dtype=torch.float64)[:2]):
        with pytest.raises(ValueError, match=rf"VqaNet.{name}: maps of shape .* for 3 questions on a 2 x 2 grid"):
            call(bad)
    with pytest.raises(ValueError, match="maps of shape"):           # the maps before the answers
        call(torch.zeros(3, 5), answers=[0, 1])
    with pytest.raises(TypeError, match="maps must be a floating tensor"):   # and before the features are looked at
        getattr(m, name)(torch.zeros(3), qfeats, [0], [0], [1]) if pairs else getattr(m, name)(torch.zeros(3), q, ql, [0, 1, 2], [1])
    # a grid above the rank kernel's cap
    big = ImageFeatures(torch.zeros(1, 8281, m._engine.C), torch.zeros(8281, m._engine.mid), (91, 91), m)
    with pytest.raises(ValueError, match=f"VqaNet.{name}: 8281 grid positions, the ranking takes at most 8192"):
        getattr(m, name)(big, qfeats, [0], [0], torch.zeros(1, 8281)) if pairs else \
            getattr(m, name)(big, q[:1], ql[:1], [0], torch.zeros(1, 91, 91))
    # everything the host can judge is in order, in every accepted form of the maps and with both caps: the device check speaks
    for fine in (GOOD, torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 2, 2, dtype=torch.float16)):
        with pytest.raises(RuntimeError, match="cuda"):
            call(fine, answers=[0, A - 1, 1], _u_bytes=64, _ws_bytes=64)
    assert m._last_ctx is None


@pytest.mark.parametrize("name,pairs,logit_name", CALLS, ids=IDS)
def test_every_refusal_is_explain_faithfulness_own_under_this_name(name, pairs, logit_name):
    g, m = tiny()
    _, other = tiny()
    m.eval(), other.eval()
    q, ql = g.t["q"][:3], g.t["q_len"][:3]

    def raised(which, feats, qfeats, index, maps, answers):
        with pytest.raises(Exception) as e:
            invoke(m, which, pairs, feats, qfeats, q, ql, index, maps, answers=answers)
        return type(e.value), str(e.value).replace(which, "CALL")

    for on_device in (False, True):
        if on_device:
            m._ensure_flat = other._ensure_flat = lambda: None
        for vprime in (True, False):
            for foreign in (False, True):
                for index in ([0, 1, 2], [0, 1], [3, 1, 2]):
                    for maps in (GOOD, torch.zeros(3, 5), torch.zeros(3, 4, dtype=torch.int32)):
                        for answers in (None, [0, 1], [0, 1, 2]):
                            theirs = host_caches(other, vprime=vprime)[0]
                            feats, qfeats = host_caches(m, vprime=vprime)
                            args = (theirs if foreign else feats, qfeats, index, maps, answers)
                            assert raised(name, *args) == raised(logit_name, *args), (on_device, vprime, foreign, index, answers)
