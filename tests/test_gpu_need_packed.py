"""st3d_need_blocks_build on bit rows (csrc/need.hip: one 64-bit word per 64 blocks of a row, the 3x3 and un-pool ORs as
shifts with a carry between words) against the numpy model tests/_needblocks_ref.py: seg, counts and list contents exactly
equal.  Sizes: S = 64 (16 blocks per row: a quarter of a word), 256 (exactly one word), 512 (two words; N = 1), and N = 2 with
different masks per image.  Masks: empty, full, one pixel at (0, 0), at (S-1, S-1), at columns 255 and 256 of S = 512 (block
columns 63 and 64: the carry), seeded blobs.  Both geometries, every nlists, with and without the run list of the relu2_1
Gram backward (from B_1)."""
import numpy as np
import pytest
import torch

import _needblocks_ref as NB
import test_gpu_need_mask as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _one(n, S, img, y, x):
    m = np.zeros((n, S, S), np.uint8)
    m[img, y, x] = 1
    return m


def _masks(n, S):
    out = {"empty": np.zeros((n, S, S), np.uint8), "full": np.ones((n, S, S), np.uint8), "first_pixel": _one(n, S, 0, 0, 0),
           "last_pixel": _one(n, S, n - 1, S - 1, S - 1), "blobs": T._blobs(n, S, 100 + S + n)}
    if S == 512:
        for x in (255, 256):
            out[f"column_{x}"] = _one(n, S, 0, 300, x)
            out[f"column_{x}_top_row"] = _one(n, S, 0, 0, x)
    if n == 2:          # the two images differ: nothing of image 0 may show in image 1's lists, nor the other way round
        mixed = T._blobs(n, S, 5 + S)
        mixed[1] = 0
        mixed[1, S - 1, 0] = 1
        out["blobs_then_one_pixel"] = mixed
        out["empty_then_full"] = np.concatenate([np.zeros((1, S, S), np.uint8), np.ones((1, S, S), np.uint8)])
    return out


def _check_list(got, ref, what):
    lst, cnt = got
    c = int(cnt)
    assert c == len(ref), (what, c, len(ref))
    assert np.array_equal(lst.cpu().numpy()[:c], ref), what
    assert bool((lst[c:] == -1).all()), (what, "entries past the count were written")


@pytest.mark.parametrize("n,S", [(1, 64), (2, 64), (1, 256), (2, 256), (1, 512)])
def test_packed_build_equals_the_numpy_model(dev, n, S):
    from st3d import ops
    nl = NB.n_lists(S)
    assert ops.need_blocks_lists(S) == nl == (3 if S == 64 else 6)
    for name, m in _masks(n, S).items():
        md = torch.from_numpy(m).to(dev)
        for cols in ([64 if (S >> NB.LIST_SHIFT[k]) % 64 == 0 else 0 for k in range(nl)], [32] * nl):
            ref = NB.need_blocks_model(m, tile_cols=cols)          # (fewer lists: the same first ones)
            for nlists in range(1, nl + 1):
                for gram in (False, True) if nlists >= 2 and (S // 2) % 64 == 0 else (False,):
                    res = ops.need_blocks_build(md, nlists=nlists, tile_cols=cols[:nlists], gram=gram)
                    what = (name, cols[0], nlists, gram)
                    assert np.array_equal(res[0].cpu().numpy(), ref["seg"]), what
                    assert len(res[1]) == nlists
                    for k in range(nlists):
                        _check_list(res[1][k], ref["lists"][k], what + (k,))
                    if gram:
                        assert res[2][0].numel() == n * (S // 2) * (S // 128)
                        _check_list(res[2], ref["gram"], what + ("relu2_1 runs",))
