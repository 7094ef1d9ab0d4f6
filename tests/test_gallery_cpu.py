"""Face gallery, the parts that need no GPU: the storage layout rfd_debug_gallery_offset states (the add kernel scatters by the
same function), and the reference restatement tests/gallery_ref.py checks itself."""
import numpy as np
import pytest

import gallery_ref as R


@pytest.mark.parametrize("dim", [32, 96, 128, 160, 352, 512, 1024])
def test_offset_is_a_bijection_for_every_multiple_of_16_rows(rfd, dim):
    """[0, rows) x [0, dim) -> [0, rows * dim) one to one, for every row count that is a multiple of 16: the first `rows` rows
    occupy exactly the first rows * dim elements, so a gallery of any capacity is a prefix of a larger one."""
    blocks = 5
    off = np.array([[rfd.gallery_offset(dim, r, d) for d in range(dim)] for r in range(16 * blocks)], np.int64)
    for b in range(1, blocks + 1):
        part = np.sort(off[:16 * b].ravel())
        assert np.array_equal(part, np.arange(16 * b * dim)), "rows %d" % (16 * b)


@pytest.mark.parametrize("dim", [32, 96, 128, 160, 352, 512, 1024])
def test_an_mfma_operand_fetch_is_one_contiguous_kib(rfd, dim):
    """The 64 lanes' B operands of one (block, K step) -- lane l: row l & 15, elements 8 * (l >> 4) .. + 7 -- lie in lane order in
    one 1 KiB span (512 bf16), 16 bytes per lane: one coalesced global_load_dwordx4 per wave."""
    for block in (0, 3):
        for ks in range(dim // 32):
            base = rfd.gallery_offset(dim, 16 * block, 32 * ks)
            assert base % 512 == 0 and base == (block * (dim // 32) + ks) * 512
            for lane in range(64):
                row, d0 = 16 * block + (lane & 15), 32 * ks + 8 * (lane >> 4)
                assert [rfd.gallery_offset(dim, row, d0 + j) for j in range(8)] == [base + 8 * lane + j for j in range(8)]


def test_offset_rejects_what_is_out_of_range(rfd):
    assert rfd.gallery_offset(48, 0, 0) == -1 and rfd.gallery_offset(2048, 0, 0) == -1
    assert rfd.gallery_offset(64, -1, 0) == -1 and rfd.gallery_offset(64, 0, 64) == -1 and rfd.gallery_offset(64, 0, -1) == -1
    assert rfd.gallery_offset(64, 5, 63) >= 0


def test_reference_rounding_is_torch_bfloat16(rfd):
    import torch
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, 4000).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, -1.0], np.float32)])
    # exact ties: 9 significant bits with the last one set, on both sides of an even / odd neighbour, both signs
    m = np.arange(256, 512, dtype=np.float64)
    ties = np.concatenate([(2 * m + 1) * 2.0 ** e for e in (-9, -20, 3)])
    x = np.concatenate([x, ties.astype(np.float32), -ties.astype(np.float32)])
    assert np.array_equal(x[-2 * len(ties):].astype(np.float64), np.concatenate([ties, -ties]))   # the ties are exact in f32
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy()
    got = R.rne_bf16(x)
    assert np.array_equal(got, want)
    assert np.count_nonzero(got[-len(ties):] != -ties) == len(ties)   # every tie moved


def test_reference_order_resolves_equal_scores_to_the_lower_row():
    rng = np.random.default_rng(5)
    g = rng.integers(-8, 9, (40, 32)).astype(np.float64) / 64
    g[31] = g[7]
    g[19] = g[7]
    q = np.stack([g[7] * 4, g[3]])
    s, r = R.topk(q, g, 5)
    full = R.scores(q, g)
    assert full[0, 7] == full[0, 19] == full[0, 31] == full[0].max()
    assert list(r[0, :3]) == [7, 19, 31] and s[0, 0] == s[0, 1] == s[0, 2]
    for i in range(2):
        keys = [(-full[i, j], j) for j in range(40)]
        assert [k[1] for k in sorted(keys)[:5]] == list(r[i])
    s, r = R.topk(q, g[:3], 5)
    assert list(r[0, 3:]) == [-1, -1] and np.all(np.isneginf(s[:, 3:])) and np.all(r[:, :3] >= 0)
