"""Inputs and fp64 references shared by tests/test_attn_bwd_long_cpu.py and tests/test_gpu_ops_attention_long_bwd.py (mmhip_op_attn_bwd_long, the
attention backward for 129..288 keys).  Pure torch on the CPU; a reference is computed once per case and never modified."""
import functools
from collections import namedtuple

import torch

import op_bounds as OB
from gpu_util import keep_mask

SEED, SID = 77, 16
S_MIN, S_MAX = 129, 288
# the launcher's tiers: ceil(S / 32) tiles spread over ceil(tiles / 4) chunks -- the chunk count steps at 128 | 129 and 256 | 257, the tile count at every
# multiple of 32.  The issue's list plus the two sizes just under a step that it does not name (255, 287)
GRID_S = [129, 160, 161, 192, 193, 197, 224, 225, 255, 256, 257, 287, 288]

Case = namedtuple("Case", "qkv64 dctx64 maskbias r")


def live_lengths(posts, S):
    """a full post, a single key, a dead tail tile, posts whose later tiles (and, from S = 161 / 257 on, whole chunks) hold no live key at all"""
    return torch.tensor(([S, 1, S - 37, 129, 33] * ((posts + 4) // 5))[:posts])


def inputs(dt, posts, S, heads, masked):
    qkv64, dctx64, _ = OB.attn_inputs(dt, posts, S, heads, False, seed=3000 * posts + S, with_dctx=True)
    maskbias = None
    if masked:
        maskbias = torch.where(torch.arange(S)[None, :] < live_lengths(posts, S)[:, None], 0.0, float("-inf")).float().contiguous()
    return qkv64, dctx64, maskbias


def reference(dt, posts, S, heads, p, masked=True, sid=SID, **kw):
    """attn_reference on the case's inputs; kw: the deliberately wrong variants (drop_last_key_of, score_scale)"""
    qkv64, dctx64, maskbias = inputs(dt, posts, S, heads, masked)
    keep, scale = (None, 1.0) if p == 0 else keep_mask((posts, heads, S, S), sid, SEED, p)
    return Case(qkv64, dctx64, maskbias, OB.attn_reference(qkv64, maskbias, posts, S, heads, keep, scale, dctx64, **kw))


@functools.lru_cache(maxsize=2)
def case(dt, posts, S, heads, p, masked=True):
    """the case as the tests share it (read only)"""
    return reference(dt, posts, S, heads, p, masked)
