"""CPU: what the 14 explain calls (VqaNet.explain, explain_integrated, explain_occlusion, explain_faithfulness,
explain_faithfulness_probs, explain_shapley, each with its _pairs form, explain_words and explain_words_occlusion) refuse before
any device work, written once over a table of the calls: bf16, train mode and the device check in that order; the type of feats
and qfeats, a bank without v', the index count and range, foreign features and the `answers` argument; and the order in which
faults that come together are judged, as one scripted table (run this module to print it: two commits compare theirs).  What only
one call asserts (the window, steps, maps, permutations / seed / orders values, the result fields, the comparisons between calls)
is in that call's own file."""
import itertools
import json

import pytest
import torch

from dl_vqa_amd import VqaNet, shapley_orders
from tests.explain_util import GOOD_MAPS, host_caches, invoke, tiny
from tests.golden_util import full_cfg

# name, pairs form, host_first (a bank without v' and the index count are judged before `answers`), maps (the call takes maps
# behind the index), an argument the call's own check refuses (bf16 and train mode are judged before it is looked at), the extra
# arguments of the device-check calls, the extra arguments of the call in which everything the host can judge is in order
CALLS = [("explain", False, False, False, {}, {}, {}),
         ("explain_pairs", True, False, False, {}, dict(answers=[0, 1, 2]), {}),
         ("explain_integrated", False, False, False, dict(steps=0), dict(steps=1), dict(steps=64, _ig_bytes=64)),
         ("explain_integrated_pairs", True, False, False, dict(steps=0), dict(answers=[0, 1, 2], steps=3), dict(steps=16)),
         ("explain_occlusion", False, False, False, dict(window=2), dict(window=3), dict(window=5)),
         ("explain_occlusion_pairs", True, False, False, dict(window=2), dict(answers=[0, 1, 2], window=7), dict(window=5)),
         ("explain_faithfulness", False, False, True, {}, {}, dict(_u_bytes=64)),
         ("explain_faithfulness_pairs", True, False, True, {}, dict(answers=[0, 1, 2]), dict(_u_bytes=64)),
         ("explain_faithfulness_probs", False, False, True, {}, {}, dict(_u_bytes=64, _ws_bytes=64)),
         ("explain_faithfulness_probs_pairs", True, False, True, {}, dict(answers=[0, 1, 2]), dict(_u_bytes=64, _ws_bytes=64)),
         ("explain_shapley", False, False, False, dict(permutations=3), dict(permutations=2), dict(permutations=256, seed=5)),
         ("explain_shapley_pairs", True, False, False, dict(permutations=3), dict(answers=[0, 1, 2], orders=[[3, 1, 0, 2]]),
          dict(orders=shapley_orders(256, 4, 1), _u_bytes=64, _ws_bytes=64)),
         ("explain_words", False, True, False, {}, {}, {}),
         ("explain_words_occlusion", False, True, False, {}, {}, dict(_variant_rows=2))]
COLUMNS, IDS = "name,pairs,host_first,maps,refused,device_kw,extra", [call[0] for call in CALLS]


@pytest.mark.parametrize(COLUMNS, CALLS, ids=IDS)
def test_bf16_then_train_mode_then_device(name, pairs, host_first, maps, refused, device_kw, extra):
    m = VqaNet(full_cfg(16), 30, compute_dtype="bf16")              # train mode, on the CPU
    q, ql = torch.ones(1, 3, dtype=torch.int64), torch.tensor([3])
    own = ("no map",) if maps else ()                               # neither the maps nor `refused` are looked at yet
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        getattr(m, name)(None, None, [0], [0], *own, **refused) if pairs else getattr(m, name)(None, q, ql, [0], *own, **refused)
    g, m = tiny()
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):
        getattr(m, name)(None, None, [0], [0], *own, **refused) if pairs else \
            getattr(m, name)(None, g.t["q"], g.t["q_len"], [0, 1, 2], *own, **refused)
    m.eval()                                                        # eval mode on the CPU: the device check speaks
    feats, qfeats = host_caches(m)
    with pytest.raises(RuntimeError, match="cuda"):
        invoke(m, name, pairs, feats, qfeats, g.t["q"][:3], g.t["q_len"][:3], [0, 1, 2], GOOD_MAPS if maps else None, **device_kw)
    assert m._last_ctx is None


@pytest.mark.parametrize(COLUMNS, CALLS, ids=IDS)
def test_features_index_and_answers_are_judged_before_any_device_work(name, pairs, host_first, maps, refused, device_kw, extra):
    g, m = tiny()
    m.eval()
    A = m._engine.A
    bank = host_caches(m, vprime=False)[0]                          # a bank without v'
    feats, qfeats = host_caches(m, N=3, M=2)
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    good = GOOD_MAPS if maps else None
    call = lambda index=(0, 1, 2), maps=good, **kw: invoke(m, name, pairs, feats, qfeats, q, ql, list(index), maps, **kw)
    own = (GOOD_MAPS,) if maps else ()
    with pytest.raises(TypeError, match="encode_images"):
        getattr(m, name)(torch.zeros(3), qfeats, [0], [0], *own) if pairs else \
            getattr(m, name)(torch.zeros(3), q, ql, [0, 1, 2], *own)
    if pairs:
        with pytest.raises(TypeError, match="encode_questions"):
            getattr(m, name)(feats, feats, [0, 1, 2], [0, 1, 1], *own) if maps else getattr(m, name)(feats, feats, [0], [0])
    if host_first:
        with pytest.raises(RuntimeError, match="with_vprime=False"):
            invoke(m, name, pairs, bank, qfeats, q, ql, [0, 1, 2])
        with pytest.raises(ValueError, match="2 image_index entries for 3 questions"):
            call(index=(0, 1))
    with pytest.raises(ValueError, match="2 answers for 3"):
        call(answers=[0, 1])
    with pytest.raises(IndexError, match=rf"answers entry {A} out of range \[0, {A}\)"):
        call(answers=[0, A, 1])
    with pytest.raises(IndexError, match="answers entry -1"):
        call(answers=torch.tensor([0, 1, -1], dtype=torch.int32))
    with pytest.raises(TypeError, match="integer"):
        call(answers=[0.0, 1.0, 2.0])
    with pytest.raises(RuntimeError, match="cuda"):                 # everything the host can judge is in order
        call(answers=[0, A - 1, 1], **extra)
    m._ensure_flat = lambda: None                                   # as on a device: the index and ownership checks speak
    with pytest.raises(ValueError, match="2 image_index entries for 3"):
        call(index=(0, 1), maps=torch.zeros(2, 2, 2) if maps and pairs else good)   # a pairs form counts its questions by the index
    with pytest.raises(IndexError):
        call(index=(0, 1, 3))
    _, other = tiny()
    with pytest.raises(RuntimeError, match="belong elsewhere"):
        invoke(m, name, pairs, host_caches(other)[0], qfeats, q, ql, [0, 1, 2], good)
    bank, qfeats = host_caches(m, vprime=False)                     # a bank without v' (the caches above are stale now)
    with pytest.raises(RuntimeError, match="with_vprime=False"):
        invoke(m, name, pairs, bank, qfeats, q, ql, [0, 1, 2], good)
    del m._ensure_flat
    feats, qfeats = host_caches(m, N=3, M=2)
    with pytest.raises(RuntimeError, match="cuda"):
        call(answers=[0, A - 1, 1], **extra)
    assert m._last_ctx is None and all(p.grad is None for p in m.parameters())


# ----------------------------------------------------------------------------- faults that come together
FAULTS = ("no v'", "index count", "answers count", "foreign features", "index out of range")


def precedence_table():
    """Every non-empty set of FAULTS against every call, twice: as a model on the CPU judges it (its parameters are not on a
    device, which VqaNet._ensure_flat says where the call reaches it), and with that one check passed, as on a device.  Returns
    {"<call> | <faults> | cpu or device": [exception type, message]}."""
    g, m = tiny()
    _, other = tiny()
    m.eval(), other.eval()
    q, ql = g.t["q"][:3], g.t["q_len"][:3]
    table = {}
    for on_device in (False, True):
        if on_device:
            m._ensure_flat = other._ensure_flat = lambda: None
        for (name, pairs, _, maps, _, _, _), n in itertools.product(CALLS, range(1, len(FAULTS) + 1)):
            for faults in itertools.combinations(FAULTS, n):
                theirs = host_caches(other, vprime="no v'" not in faults)[0]
                feats, qfeats = host_caches(m, vprime="no v'" not in faults)
                feats = theirs if "foreign features" in faults else feats
                index = [3, 1, 2] if "index out of range" in faults else [0, 1, 2]
                index = index[:2] if "index count" in faults else index
                answers = [0, 1] if "answers count" in faults else [0, 1, 2]
                with pytest.raises(Exception) as e:
                    invoke(m, name, pairs, feats, qfeats, q, ql, index, GOOD_MAPS if maps else None, answers=answers)
                table[f"{name} | {', '.join(faults)} | {'device' if on_device else 'cpu'}"] = [type(e.value).__name__, str(e.value)]
    return table


def test_every_set_of_faults_is_refused_on_the_host_in_the_calls_own_name():
    table = precedence_table()
    assert len(table) == 2 * len(CALLS) * (2 ** len(FAULTS) - 1)
    for cell, (kind, message) in table.items():
        name, faults, where = cell.split(" | ")
        assert kind in ("ValueError", "IndexError", "RuntimeError"), cell
        if where == "device":                                       # a fault speaks, never the device check
            assert message.startswith(f"VqaNet.{name}: ") or (kind == "IndexError" and "index out of range" in faults), cell


if __name__ == "__main__":                                          # python -m tests.test_explain_refusals_cpu > table.json
    print(json.dumps(precedence_table(), indent=1, sort_keys=True))
