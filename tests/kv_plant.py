"""Planted KV caches for the attention key-range tests (tests/test_oracle_plant.py on the CPU, tests/test_hip_attn_keyrange.py on the GPU).  No GPU code.

On the synthetic checkpoints the softmax is nearly uniform: one key among n carries ~1/n of a head's output, and a kernel that loses or gains one key at a tile
edge moves the logits by less than any logits tolerance once n is a few hundred.  plant() rewrites a cache so that every key at an edge counts:
  loud V     the V rows at boundary_keys(L) become +-A, the sign by (position, dim), A a power of two >= L * max|v|: a key of weight ~1/L then contributes as much
             as all plain keys together, and each loud key with its own sign pattern, so losing one, gaining one or swapping two all show;
  uneven K   the K rows at positions = K_RESIDUE (mod K_PERIOD) are multiplied by K_FACTOR (a power of two): their scores spread K_FACTOR times as wide, the running
             maximum moves from tile to tile, and the online-softmax rescale and the split merge do real work.
Every planted value is a power of two times a stored value (or +-A itself): exactly representable in bf16 and fp16, so write_kv's rounding is the identity on them.
A and the K factor are CHOSEN by tests/test_oracle_plant.py's sensitivity sweep (the oracle with one key ablated against itself), not by any GPU result."""
import copy

import numpy as np

TILE = 64           # the finest key tile of any attention form; the 128-key split blocks, the 128-token paged blocks and the 192 / 384 / 576 form limits are multiples
K_PERIOD, K_RESIDUE, K_FACTOR = 13, 5, 4.0
LOUD_GAIN = 1.0
POISON = 4096.0     # 2^12: finite in every storage dtype

# every length the decode forms are held at: around each multiple of 64 up to 576, the 192 / 384 / 576 limits among them, and one length that is no multiple of anything
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513, 575, 576, 577, 645]
MODELS = ["llama-3.2-1b", "mistral-7b-v0.3", "qwen2.5-0.5b"]      # head_dim 64, G = 4; head_dim 128; G = 7 with QKV bias


def cut_desc(name, dtype="bf16", max_ctx=768, max_batch=1, layers=2):
    """the 2-layer, vocab-4096 cut of a released geometry the row tests use"""
    from tinygpt_amd import known_desc
    d = copy.deepcopy(known_desc(name, dtype))
    d.layers, d.vocab, d.max_ctx, d.max_batch = layers, 4096, max_ctx, max_batch
    return d


def boundary_keys(L):
    """{0, L-2, L-1} and {b-1, b} for every multiple b of TILE below L (what lies in [0, L))"""
    keys = {0, L - 2, L - 1}
    for b in range(TILE, L, TILE):
        keys |= {b - 1, b}
    return sorted(p for p in keys if 0 <= p < L)


def scaled_keys(L):
    """the positions = K_RESIDUE (mod K_PERIOD) below L that are no boundary key: 447 and 512 are both, and a loud key with a 4x score takes the softmax from every
    other loud key in the heads where its score is positive (the sweep measured 1e-3 instead of 1e-1 for keys 64 and 255 at L = 513 / 645) — the K plant moves"""
    bk = set(boundary_keys(L))
    return [p for p in range(K_RESIDUE, L, K_PERIOD) if p not in bk]


def loud_sign(pos, n):
    """+-1 per (position, flattened dim): a multiplicative hash, so two positions never share a pattern"""
    pos = np.asarray(pos, dtype=np.uint64).reshape(-1, 1)
    dim = np.arange(n, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):      # (uint64 wrap-around is the hash)
        h = pos * np.uint64(0x9E3779B97F4A7C15) + dim * np.uint64(0xBF58476D1CE4E5B9)
        h = (h ^ (h >> np.uint64(31))) * np.uint64(0x94D049BB133111EB)
        h = h ^ (h >> np.uint64(29))
    return (1.0 - 2.0 * ((h >> np.uint64(40)) & np.uint64(1)).astype(np.float32)).astype(np.float32)


def loud_amplitude(v, L):
    """the power of two at or above L * max|v|"""
    vmax = float(np.abs(np.asarray(v[:L], np.float32)).max())
    return float(2.0 ** int(np.ceil(np.log2(max(LOUD_GAIN * L * vmax, 1.0)))))


def plant(k, v, L):
    """k, v: fp32 [>= L][kv_heads][head_dim] as read_kv returns them -> planted copies of rows [0, L)"""
    k = np.array(k[:L], dtype=np.float32, copy=True)
    v = np.array(v[:L], dtype=np.float32, copy=True)
    A = loud_amplitude(v, L)
    bk = boundary_keys(L)
    v[bk] = (A * loud_sign(bk, v.shape[1] * v.shape[2])).reshape((len(bk),) + v.shape[1:])
    k[scaled_keys(L)] *= np.float32(K_FACTOR)
    return k, v


def poison(shape):
    """+-2^12, alternating by element: finite stale data (the caches are zeroed at creation, so a masked 0 * stale is legitimate and only finite data can occur)"""
    n = int(np.prod(shape))
    return np.where(np.arange(n) % 2 == 0, np.float32(POISON), np.float32(-POISON)).astype(np.float32).reshape(shape)


def synthetic_rows(desc, n, seed):
    """cache rows with the statistics of the synthetic checkpoints' own (K after RoPE and V are ~N(0, 1) there), already rounded to bf16: the base the CPU sweep plants
    into, so that the oracle never has to prefill"""
    from tinygpt_amd.synth import bf16_bits_to_f32, f32_to_bf16_bits
    rng = np.random.default_rng(seed)
    out = []
    for layer in range(desc.layers):
        kv = rng.standard_normal((2, n, desc.kv_heads, desc.head_dim)).astype(np.float32)
        kv = bf16_bits_to_f32(f32_to_bf16_bits(kv)).reshape(kv.shape)
        out.append((kv[0], kv[1]))
    return out


def onehot(tok, vocab, rows=1):
    """the set_logits idiom: logits whose greedy sample is `tok`"""
    toks = np.asarray(tok, dtype=np.int64).reshape(-1)
    l = np.full((len(toks), vocab), -1.0, np.float32)
    l[np.arange(len(toks)), toks] = 1.0
    return l
