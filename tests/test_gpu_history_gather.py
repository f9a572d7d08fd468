"""GPU: the one history gather of the sequence towers (gather._history_rows).  Every tower gives the same query and the same
item-table gradient whether the batch carries the device loader's CSR view (``_seg``: rsa_seg_gather) or only the padded ids
(rsa_embedding_gather): the gather copies rows and the backward is the same sorted, atomics-free scatter over the same ids, so the
bar is ``torch.equal``.  And the mask token of CL4SRec's tower never reaches a catalog row."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, D, B, L = 50, 64, 5, 8
SEQLEN = [1, 3, 8, 8, 5]


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


def histories():
    """[B, L] right-padded with 0; history 2 holds item 7 three times (a run for the sorted scatter); plus the CSR view."""
    g = torch.Generator().manual_seed(11)
    hist = torch.randint(1, N, (B, L), generator=g)
    hist[2, [1, 4, 6]] = 7
    seqlen = torch.tensor(SEQLEN)
    hist[torch.arange(L).view(1, -1) >= seqlen.view(-1, 1)] = 0
    flat = torch.cat([hist[b, :n] for b, n in enumerate(SEQLEN)])
    end = torch.cumsum(seqlen, 0)
    assert int(end[-1]) == flat.numel() == sum(SEQLEN) and int((hist[2] == 7).sum()) == 3
    return hist, seqlen, (flat, end - seqlen, end)


def tower(name, item):
    from recstudio_amd import models_seq as ms
    if name in ('sasrec', 'sasrec_fused'):
        return ms.SASRecQueryEncoder('item_id', D, L, 2, 128, 0.5, 'gelu', 1e-12, 2, item, fused_attention=name == 'sasrec_fused')
    if name == 'gru4rec':
        return ms.GRU4RecQueryEncoder('item_id', D, 128, 0.3, 1, item)
    if name == 'narm':
        return ms.NARMQueryEncoder('item_id', D, 128, 1, [0.25, 0.5], item)
    if name == 'stamp':
        return ms.STAMPQueryEncoder('item_id', D, item)
    return ms.HGNQueryEncoder('user_id', 'item_id', 9, D, L, item)


@pytest.mark.parametrize('name', ['sasrec', 'sasrec_fused', 'gru4rec', 'narm', 'stamp', 'hgn'])
def test_csr_view_and_padded_ids_give_the_same_query_and_gradient(ra, name):
    torch.manual_seed(4)
    item = torch.nn.Embedding(N, D, padding_idx=0)
    enc = tower(name, item).to(DEV).eval()
    hist, seqlen, seg = histories()
    batch = {'in_item_id': hist.to(DEV), 'seqlen': seqlen.to(DEV), 'user_id': torch.arange(1, B + 1, device=DEV)}
    runs = []
    for with_seg in (True, False):
        item.weight.grad = None
        out = enc(dict(batch, _seg=tuple(t.to(DEV) for t in seg)) if with_seg else batch)
        out.sum().backward()
        runs.append((out.detach().clone(), item.weight.grad.clone()))
    (q_seg, g_seg), (q_ids, g_ids) = runs
    print(name, 'max |dq|', float((q_seg - q_ids).abs().max()), 'max |dg|', float((g_seg - g_ids).abs().max()))
    assert q_seg.shape == (B, D) and bool(torch.isfinite(q_seg).all()) and bool(g_seg.any()) and not bool(g_seg[0].any())
    assert torch.equal(q_seg, q_ids)
    assert torch.equal(g_seg, g_ids)


def test_mask_token_goes_to_mask_emb_not_to_a_catalog_row(ra):
    from recstudio_amd.models_seq import SASRecQueryEncoder
    torch.manual_seed(4)
    item = torch.nn.Embedding(N, D, padding_idx=0)
    enc = SASRecQueryEncoder('item_id', D, L, 2, 64, 0.5, 'gelu', 1e-12, 1, item, mask_id=N).to(DEV).eval()
    with torch.no_grad():
        enc.mask_emb.normal_()
    hist, seqlen, _ = histories()
    hist[2, 0] = hist[3, 5] = hist[4, 1] = N                       # inside the histories, in front of the last position
    out = enc({'in_item_id': hist.to(DEV), 'seqlen': seqlen.to(DEV)})
    out.sum().backward()
    assert out.shape == (B, D) and bool(torch.isfinite(out).all())
    assert bool(torch.isfinite(item.weight.grad).all()) and not bool(item.weight.grad[0].any())
    assert bool(enc.mask_emb.grad.any())
