"""The numpy reference of tgx_embed_rows' pooling (include/tgx.h), in float64, and the identity-head checkpoint that lets the CPU oracle show its final-normed
hidden rows: an untied lm_head whose first H rows are the identity makes logits[:H] the row lm_head is multiplied with (the tail logits are exactly 0)."""
import numpy as np

POOLS = ("last", "mean", "first")


def pool_ref(hidden, pool="last", normalize=True, dims=0):
    """hidden [len][H] final-normed rows of one text -> the float64 vector of tgx_embed_rows: pool, keep the first dims components, then L2-normalise"""
    h = np.asarray(hidden, dtype=np.float64)
    assert h.ndim == 2 and len(h) >= 1 and pool in POOLS
    v = h[-1] if pool == "last" else (h[0] if pool == "first" else h.sum(axis=0) / len(h))
    if dims:
        assert 1 <= dims <= h.shape[1]
        v = v[:dims]
    if normalize:
        n = np.sqrt((v * v).sum())
        v = v / n if n > 0 else v
    return v


def identity_head(desc, tensors):
    """`tensors` (name -> bf16 bits of a synthetic checkpoint of the UNTIED desc) with lm_head.weight replaced by the identity on its first H rows"""
    H, V = desc.hidden, desc.vocab
    assert not desc.tied and V >= H, "the identity head needs an untied lm_head of at least hidden rows"
    t = dict(tensors)
    head = np.zeros((V, H), dtype=np.uint16)
    head[np.arange(H), np.arange(H)] = 0x3F80      # bf16 bits of 1.0
    t["lm_head.weight"] = head
    return t
