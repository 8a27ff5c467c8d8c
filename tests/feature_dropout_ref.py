"""Float64 reference of vqa_gather_rows_drop_norm (include/vqa_hip.h): image dropout on the asked rows of a bank of
L2-normalised image features, the rows renormalised after the mask.  The masks are DATA (keep-scale masks of the whole
bank: 0 or 1/(1-p) per element), so the reference knows nothing of the dropout RNG; a GPU test extracts them with
ops.dropout on ones of the bank, as tests/hip_masks.py does.  Also the two orders of the identity the feature rests on:
`l2norm` (what the bank holds) and `oracle_drop_then_norm` (what the reference model computes, models/model.py:55-56).
`relu_margins`: how far the float64 oracle's ReLU pre-activations are from zero on a batch, which decides whether gradients
can be compared on it at all."""
import torch

EPS = 1e-12


def l2norm(x):
    """x / (|x| + 1e-12) over the last axis: what encode_images caches."""
    x = x.double()
    return x / (x.norm(dim=-1, keepdim=True) + EPS)


def oracle_drop_then_norm(pooled, mask_img):
    """The reference's order: image.drop on the pooled features, then v / (|v| + 1e-12)."""
    return l2norm(pooled.double() * mask_img.double())


def drop_norm(bank, rows, mask_img, mask_att=None):
    """bank [M, P, C]; rows: integers [n], an entry outside [0, M) gives zeros; mask_img, mask_att [M, P, C] keep-scale masks
    indexed by the BANK row.  Returns vn_out [n, P, C] float64, or (vn_out, vdrop_out) when mask_att is given:
        u = bank[r] * mask_img[r];  vn_out = u * (1 / (|u| + 1e-12));  vdrop_out = vn_out * mask_att[r]."""
    bank = bank.double()
    M, P, C = bank.shape
    rows = torch.as_tensor(rows).long().reshape(-1)
    inside = (rows >= 0) & (rows < M)
    r = rows.clamp(0, M - 1)
    u = bank[r] * mask_img.double()[r]
    vn = u * (1.0 / (u.norm(dim=-1, keepdim=True) + EPS))
    vn = vn * inside.double()[:, None, None]
    if mask_att is None:
        return vn
    return vn, vn * mask_att.double()[r]


def relu_margins(sd, cfg, pooled, image_index, q, q_len, masks, device="cpu"):
    """How far the float64 oracle's ReLU pre-activations behind the image encoder are from zero, for one train-mode batch:
    (min |v' + q'| over the attention stage's [B, mid, P] pre-activations, min |lin1 pre-activation| of the classifier).
    A parameter gradient is discontinuous where such a value crosses zero, so a comparison of gradients with the oracle
    judges the arithmetic only on a batch whose margins exceed the fp32 error of those values.  pooled [N, C, g, g]: the
    oracle's image-encoder output for the N images of the bank, masks: the sites as data, one row per question.
    do_option '+' (the north-star configuration).  device: where the large products run."""
    from oracle import vqa_oracle as O
    assert cfg["attention"]["do_option"] == "+"
    vn = O.l2_normalise(pooled.double()[image_index] * masks["image"].double())
    qf = O.question_encoder(sd, q, q_len, cfg["text"]["bidirectional"], masks)
    d = lambda t: t.double().to(device)
    wv = d(sd["attention.v_conv.weight"])[:, :, 0, 0]
    vv = torch.einsum("bchw,mc->bmhw", d(vn) * d(masks["att_v"]), wv)
    qq = (d(qf) * d(masks["att_q"])) @ d(sd["attention.q_lin.weight"]).t() + d(sd["attention.q_lin.bias"])
    x_pre = vv + qq[:, :, None, None]
    att = torch.einsum("bmhw,gm->bghw", torch.relu(x_pre) * d(masks["att_x"]), d(sd["attention.x_conv.weight"])[:, :, 0, 0]) \
        + d(sd["attention.x_conv.bias"])[None, :, None, None]
    wsum, _ = O.image_question_attention(d(vn), att)
    comb = torch.cat([wsum, d(qf)], dim=1) * d(masks["cls1"])
    h_pre = comb @ d(sd["classifier.lin1.weight"]).t() + d(sd["classifier.lin1.bias"])
    return float(x_pre.abs().min()), float(h_pre.abs().min())


def kept_norms(bank, rows, mask_img):
    """|bank[r] * (mask_img[r] != 0)| per compared feature row [n_inside, P]: what the tests bound away from 1e-12."""
    M = bank.shape[0]
    rows = torch.as_tensor(rows).long().reshape(-1)
    r = rows[(rows >= 0) & (rows < M)]
    return (bank.double()[r] * (mask_img[r] != 0).double()).norm(dim=-1)
