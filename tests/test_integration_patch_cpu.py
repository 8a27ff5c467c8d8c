"""CPU: the patch INTEGRATION.md documents for the reference's train.py really swaps in the fused run_batch.

Round-2 ADVICE: an `import run_batch` at the top of the reference's train.py is a no-op, because that file
defines its own module-level `def run_batch` further down (train.py:172) and `train()` / `evaluate()` look the
name up at call time (train.py:70,159).  The documented patch therefore appends the import at the END of the file.
Two checks:
  1. the name-binding rule itself, on a synthetic module of the same shape;
  2. the patched loop shape end to end on the CPU stand-in engine: run_batch -> zero_grad -> update_learning_rate
     -> backward -> step (train.py:70-80), with FusedAdam, and under data parallelism (gloo, world_size 2) with
     NO explicit divisor -- the global-batch divisor must come from the attached synchroniser.
"""
import os
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_autograd_glue_cpu import _free_port, close, make_model, oracle_grads

PATCH_TAIL = "from dl_vqa_amd.train import run_batch, FusedAdam   # noqa: E402,F811\n"


def test_an_import_at_the_end_of_the_module_wins_and_one_at_the_top_does_not():
    body = ("def train(x):\n    return run_batch(x)\n\n"
            "def run_batch(x):\n    return 'reference'\n")
    top = types.ModuleType("patched_top")
    exec(compile(PATCH_TAIL + body, "patched_top", "exec"), top.__dict__)
    assert top.train(1) == "reference"                       # the round-2 doc: silently still the host-side loss
    end = types.ModuleType("patched_end")
    exec(compile(body + PATCH_TAIL, "patched_end", "exec"), end.__dict__)
    from dl_vqa_amd.train import run_batch
    assert end.run_batch is run_batch


def _cpu_softce(monkeypatch_target):
    """dl_vqa_amd.train's loss head on the CPU: the oracle's soft-target CE / score in place of the HIP kernel."""
    from oracle import vqa_oracle as O

    def soft_ce_loss_and_score(logits, a_indices, a_values, batch_divisor=None):
        div = float(batch_divisor if batch_divisor is not None else logits.shape[0])
        loss = O.soft_ce_loss(logits, a_indices, a_values) * (logits.shape[0] / div)
        return loss, O.batch_accuracy(logits.detach(), a_indices, a_values)
    monkeypatch_target.soft_ce_loss_and_score = soft_ce_loss_and_score


def _reference_shaped_loop(model, batches, lr, run_batch, FusedAdam, update_learning_rate, max_answers=12):
    """train.py:55-80 with the documented patch applied (FusedAdam instead of torch.optim.Adam; run_batch the fused one)."""
    optimizer = FusedAdam(model, lr=lr)
    total_iterations = 0
    for batch_data in batches:
        batch_loss, batch_score = run_batch(model, None, batch_data, max_answers)
        optimizer.zero_grad()
        update_learning_rate(optimizer=optimizer, iteration=total_iterations, initial_lr=lr)
        batch_loss.backward()
        optimizer.step()
        total_iterations += 1
    return optimizer


def _patch_cpu(tr, ops):
    from oracle import vqa_oracle as O
    _cpu_softce(tr)

    def cpu_adam(p, g, m1, m2, lr, step, b1, b2, eps, grad_scale=1.0):
        O.adam_step(p, g * grad_scale, m1, m2, step, lr, b1, b2, eps)
    ops.adam = cpu_adam


def test_patched_loop_matches_oracle_adam_steps(monkeypatch):
    from dl_vqa_amd import ops
    from dl_vqa_amd import train as tr
    from oracle import vqa_oracle as O
    monkeypatch.setattr(tr, "soft_ce_loss_and_score", tr.soft_ce_loss_and_score)
    monkeypatch.setattr(ops, "adam", ops.adam)
    _patch_cpu(tr, ops)
    m, cfg = make_model(seed=7)
    batches = [O.synthetic_batch(4, 32, 5, 40, 12, seed=s) for s in (1, 2)]
    sd = {k: p.data.clone() for k, p in m.named_parameters()}
    mom = {k: (torch.zeros_like(t), torch.zeros_like(t)) for k, t in sd.items()}
    _reference_shaped_loop(m, batches, 1e-3, tr.run_batch, tr.FusedAdam, tr.update_learning_rate)
    for it, b in enumerate(batches):
        v, q, a_idx, a_val, _, _, q_len = b
        grads = O.loss_and_grads(sd, cfg, v, q, q_len, a_idx, a_val)[2]
        for k in sd:
            O.adam_step(sd[k], grads[k], mom[k][0], mom[k][1], it + 1, O.learning_rate(1e-3, it))
    for n, p in m.named_parameters():
        close(p.data, sd[n], n)


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dl_vqa_amd import ops
        from dl_vqa_amd import train as tr
        from dl_vqa_amd.distributed import DataParallel, shard_batch
        from oracle import vqa_oracle as O
        _patch_cpu(tr, ops)
        m, cfg = make_model(seed=30 + rank)
        DataParallel(m)
        g = O.synthetic_batch(4, 32, 5, 40, 12, seed=8)
        # the reference's call: no divisor argument (train.py:70-73)
        loss, _ = tr.run_batch(m, None, shard_batch(g, rank, world), 12)
        loss.backward()
        torch.save({"loss": loss.detach().clone(), "grads": {n: p.grad.clone() for n, p in m.named_parameters()}},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_run_batch_uses_the_global_batch_divisor_under_data_parallelism(tmp_path):
    from oracle import vqa_oracle as O
    world, port = 2, _free_port()
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    m, cfg = make_model(seed=30)
    g = O.synthetic_batch(4, 32, 5, 40, 12, seed=8)
    v, q, a_idx, a_val, _, _, q_len = g
    sd = {k: p.data.clone() for k, p in m.named_parameters()}
    _, loss_ref, grads_ref = O.loss_and_grads(sd, cfg, v, q, q_len, a_idx, a_val)
    assert abs(float(r0["loss"] + r1["loss"]) - float(loss_ref)) < 1e-5      # local losses sum to the global mean
    for n, ref in grads_ref.items():
        assert torch.equal(r0["grads"][n], r1["grads"][n]), n
        close(r0["grads"][n], ref, n)                                         # = one GPU on the whole batch
