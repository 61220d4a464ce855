"""CPU: the host-side rules of per-image visual prompts (GRIP_FWD_PER_IMAGE_PREFIX): which prompt shapes are shared, which are per image,
which raise (the reference's image_prefix.expand(B, -1, -1), models/clip_encoders.py:148), and the refine tiers' row gather."""
import os
import re
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tower(width=8):
    return types.SimpleNamespace(width=width)


def test_prompt_shapes_follow_expand():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    t = _tower()
    vit_prefix = engine.Tower.vit_prefix
    assert vit_prefix(t, None, 4) == (None, 0, False)
    p, P, per = vit_prefix(t, torch.ones(3, 8, dtype=torch.float16), 4)
    assert (p.shape, p.dtype, P, per) == ((3, 8), torch.float32, 3, False)
    p, P, per = vit_prefix(t, torch.ones(1, 3, 8), 4)
    assert (p.shape, P, per) == ((3, 8), 3, False)
    x = torch.arange(4 * 3 * 8, dtype=torch.float32).reshape(4, 3, 8)
    p, P, per = vit_prefix(t, x.transpose(0, 1).contiguous().transpose(0, 1), 4)
    assert (p.shape, P, per) == ((4, 3, 8), 3, True) and p.is_contiguous() and torch.equal(p, x)
    for bad in (torch.ones(2, 3, 8), torch.ones(5, 3, 8), torch.ones(4, 3, 7)):
        with pytest.raises(native.GripError, match="one prompt per image"):
            vit_prefix(t, bad, 4)
    assert engine.is_per_image_prefix(torch.ones(4, 3, 8)) and not engine.is_per_image_prefix(torch.ones(1, 3, 8))
    assert not engine.is_per_image_prefix(torch.ones(3, 8)) and not engine.is_per_image_prefix(None)


def test_take_prefix_gathers_the_rows_prompts():
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
    prompts = torch.arange(10 * 2 * 4, dtype=torch.float32).reshape(10, 2, 4)
    idx = np.array([1, 4, 9], dtype=np.int64)
    assert torch.equal(pl.take_prefix(prompts, idx), prompts[[1, 4, 9]])
    shared = torch.ones(2, 4)
    assert pl.take_prefix(shared, idx) is shared and pl.take_prefix(None, idx) is None
    assert pl.take_prefix(shared[None], idx).shape == (1, 2, 4)


def test_flag_and_abi_match_the_header():
    import grip_amd  # noqa: F401
    from grip_amd import native
    with open(os.path.join(REPO, "include", "grip_amd.h")) as f:
        h = f.read()
    assert int(re.search(r"#define GRIP_FWD_PER_IMAGE_PREFIX (\d+)", h).group(1)) == native.FWD_PER_IMAGE_PREFIX == 32
    assert int(re.search(r"#define GRIP_ABI_VERSION (\d+)", h).group(1)) == native.ABI_VERSION == 9
    flags = [int(v) for v in re.findall(r"#define GRIP_FWD_\w+ (\d+)", h)]
    assert 16 not in flags and len(set(flags)) == len(flags)
