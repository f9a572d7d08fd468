"""GPU: ops.seq_augment (rsa_seqaug.hip) against data_augmentation.seq_augment_torch fed torch.rand([B, L + 1]) from the same
generator state, and against the per-sequence referee of tests/seq_augment_referee.py: ids, lengths and the generator offset."""
import pytest
import torch

import seq_augment_referee as sa

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MASK_ID = 12345
OUTSIDE = 777777                                                          # fills the buffer around the view: never an output


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


def offset():
    return torch.cuda.default_generators[torch.cuda.current_device()].get_offset()


def histories(B, L, seed, dtype=torch.int64):
    """``seq`` as a VIEW inside a wider buffer filled with an out-of-range id; lengths 0, 1, L and mixed."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, L + 1, (B,), generator=g)
    lens[:3] = torch.tensor([L, 0, 1])[:B]
    ids = torch.randint(1, 10000, (B, L), generator=g)
    ids = ids * (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1))
    buf = torch.full((B + 2, L + 7), OUTSIDE, dtype=torch.int64)
    buf[1:B + 1, 3:3 + L] = ids
    buf = buf.to(DEV)
    return buf[1:B + 1, 3:3 + L], lens.to(dtype).to(DEV)


@pytest.mark.parametrize('kind', sa.KINDS)
@pytest.mark.parametrize('B,L', [(1, 1), (3, 9), (5, 20), (2, 50), (2, 64), (300, 20), (70000, 20)])
def test_kernel_equals_twin(ra, B, L, kind):
    da = ra.data_augmentation
    if B == 70000:
        cu, mt = ra.rng.device_props(DEV)
        assert B * (L + 1) > ra.rng.grid_threads(B * (L + 1), cu, mt)     # elements past the first Philox round of the grid
    for rate, len_dtype in ((0.7, torch.int64), (0.2, torch.int32), (1.0, torch.int64)):
        seq, lens = histories(B, L, 31 * B + L, len_dtype)
        assert not seq.is_contiguous() or B == 1
        sub = da.sub_table(kind, rate, L, DEV)
        torch.manual_seed(5)
        out, new_len = ra.ops.seq_augment(seq, lens, kind, sub, MASK_ID)
        after = offset()
        torch.manual_seed(5)
        U = torch.rand(B, L + 1, device=DEV)
        assert offset() == after                                          # the generator is where that torch call leaves it
        want, want_len = da.seq_augment_torch(seq, lens, kind, sub, U, MASK_ID)
        assert out.dtype == torch.int64 and new_len.dtype == len_dtype and out.is_contiguous()
        assert torch.equal(out, want) and torch.equal(new_len, want_len)
        assert not bool((out == OUTSIDE).any())                           # nothing outside the view is read into the output
        torch.manual_seed(5)
        again, again_len = ra.ops.seq_augment(seq, lens, kind, sub, MASK_ID)
        assert torch.equal(out, again) and torch.equal(new_len, again_len)
        if B <= 300:                                                      # and the per-sequence referee itself
            ref, ref_len = sa.augment(seq.cpu().numpy(), lens.cpu().numpy(), kind, sa.sub_lengths(kind, rate, L), U.cpu().numpy(), MASK_ID)
            assert torch.equal(out.cpu(), torch.from_numpy(ref)) and torch.equal(new_len.cpu().long(), torch.from_numpy(ref_len))
        if kind != 'crop' or rate < 1.0:
            assert B < 300 or not torch.equal(out, seq)


def test_modules_and_fallback(ra):
    da = ra.data_augmentation
    seq, lens = histories(40, 20, 3)
    for fused_mod, twin_mod in ((da.Item_Crop(0.5), da.Item_Crop(0.5, fused=False)), (da.Item_Mask(MASK_ID), da.Item_Mask(MASK_ID, fused=False)),
                                (da.Item_Reorder(0.8), da.Item_Reorder(0.8, fused=False))):
        torch.manual_seed(9)
        a = fused_mod(seq, lens)
        end = offset()
        torch.manual_seed(9)
        b = twin_mod(seq, lens)
        assert offset() == end and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a generator of the caller's
    g = torch.Generator(device=DEV).manual_seed(9)
    own = da.Item_Reorder(0.8)(seq, lens, generator=g)
    assert torch.equal(own[0], a[0]) and g.get_offset() > 0
    # L = 70: above the kernel's 64 positions the module runs the twin; the kernel's wrapper refuses
    seq, lens = histories(6, 70, 4)
    torch.manual_seed(2)
    out, new_len = da.Item_Mask(MASK_ID)(seq, lens)
    torch.manual_seed(2)
    U = torch.rand(6, 71, device=DEV)
    ref, ref_len = sa.augment(seq.cpu().numpy(), lens.cpu().numpy(), 'mask', sa.sub_lengths('mask', 0.7, 70), U.cpu().numpy(), MASK_ID)
    assert torch.equal(out.cpu(), torch.from_numpy(ref)) and torch.equal(new_len.cpu(), torch.from_numpy(ref_len))
    with pytest.raises(ValueError, match='L must lie'):
        ra.ops.seq_augment(seq, lens, 'mask', da.sub_table('mask', 0.7, 70, DEV), MASK_ID)
    empty = ra.ops.seq_augment(seq[:0, :20], lens[:0], 'crop', da.sub_table('crop', 0.2, 20, DEV))
    assert empty[0].shape == (0, 20) and empty[1].shape == (0,)
