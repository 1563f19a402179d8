"""A numpy reference of tgx_splice_row's move (include/tgx.h): V rows move, K rows move and are rotated by the difference of two table angles.  The angles are the
float32 values the library's RoPE tables take cosf / sinf of — inv[i] = 1 / fl32(theta ** fl32(2 i / hd)), angle[p][i] = fl32(inv[i] * fl32(p)), formed as
build_rope_host (csrc/abi.hip) forms them, for the families with unscaled frequencies — and the rotation itself is done in fp64, with no storage rounding."""
import numpy as np


def inv_freq(desc) -> np.ndarray:
    assert desc.family != "gpt2" and not desc.rope_factor > 0, "unscaled RoPE frequencies only"
    hd = desc.head_dim
    e = (2 * np.arange(hd // 2)).astype(np.float32) / np.float32(hd)
    p = np.power(np.float64(np.float32(desc.rope_theta)), e.astype(np.float64)).astype(np.float32)
    return (np.float32(1.0) / p).astype(np.float32)


def angles(desc, n: int) -> np.ndarray:
    """float32 [n][hd / 2]"""
    return (inv_freq(desc)[None, :] * np.arange(n, dtype=np.float32)[:, None]).astype(np.float32)


def segments(ranges):
    """(src, dst, len) of every kept range"""
    out, kept = [], 0
    for s, n in ranges:
        out.append((int(s), kept, int(n)))
        kept += int(n)
    return out


def source_positions(ranges) -> np.ndarray:
    return np.concatenate([np.arange(s, s + n) for s, n in ranges])


def splice(k: np.ndarray, v: np.ndarray, ranges, ang: np.ndarray):
    """k, v [T][kv_heads][hd] -> the spliced (k', v') [new_len][kv_heads][hd] in fp64; rows with delta == 0 are copies"""
    src = source_positions(ranges)
    dst = np.arange(len(src))
    half = k.shape[-1] // 2
    ks = k[src].astype(np.float64)
    a = (ang[dst].astype(np.float64) - ang[src].astype(np.float64))[:, None, :]      # [new_len][1][half]
    c, s = np.cos(a), np.sin(a)
    x0, x1 = ks[..., :half], ks[..., half:]
    out = np.concatenate([x0 * c - x1 * s, x1 * c + x0 * s], axis=-1)
    same = src == dst
    out[same] = ks[same]
    return out, v[src].astype(np.float64)


def pair_norm(k: np.ndarray) -> np.ndarray:
    """the norm of the (p, p + hd/2) pair an entry belongs to, in the entry's place"""
    half = k.shape[-1] // 2
    n = np.sqrt(k[..., :half].astype(np.float64) ** 2 + k[..., half:].astype(np.float64) ** 2)
    return np.concatenate([n, n], axis=-1)
