"""Packed documents on the CPU path: the packing helpers, attention_reference(key_start=...) against
per-document causal attention, and a packed llama_tiny row against its documents run one by one."""
import pytest
import torch

from kubeml_amd.nn.transformer import attention_reference, doc_key_start, pack_documents


def test_pack_documents_and_key_start():
    doc = torch.tensor([[0, 0, 0, 1, 2, 2, 3], [5, 5, 5, 5, 5, 5, 5], [4, 0, 4, 4, 0, 0, 1]])
    ks = doc_key_start(doc)
    assert ks.dtype == torch.int32 and ks.tolist() == [[0, 0, 0, 3, 4, 4, 6], [0] * 7, [0, 1, 2, 2, 4, 4, 6]]
    with pytest.raises(ValueError):
        doc_key_start(doc.float())
    docs = [torch.arange(1, 4), torch.arange(10, 22), torch.arange(30, 32), torch.arange(40, 43), torch.arange(50, 51)]
    ids, mask, doc = pack_documents(docs, 5, pad_id=99)
    # [1 2 3] alone (the next piece does not fit); the 12-token document cut into 5 + 5 + 2, its rest
    # sharing a row with [30 31]; [40 41 42] and [50] share the last row; padding is a document
    assert ids.tolist() == [[1, 2, 3, 99, 99], [10, 11, 12, 13, 14], [15, 16, 17, 18, 19], [20, 21, 30, 31, 99],
                            [40, 41, 42, 50, 99]]
    assert mask.tolist() == [[1, 1, 1, 0, 0], [1] * 5, [1] * 5, [1, 1, 1, 1, 0], [1, 1, 1, 1, 0]]
    assert doc.tolist() == [[0, 0, 0, 1, 1], [0] * 5, [0] * 5, [0, 0, 1, 1, 2], [0, 0, 0, 1, 2]]
    assert doc_key_start(doc).tolist() == [[0, 0, 0, 3, 3], [0] * 5, [0] * 5, [0, 0, 2, 2, 4], [0, 0, 0, 3, 4]]


@pytest.mark.parametrize("D", [64, 128])
def test_reference_key_start_is_per_document_attention(D):
    B, H, Hkv, lens = 2, 4, 2, [3, 1, 4]
    L = sum(lens)
    qkv = torch.randn(B * L, (H + 2 * Hkv) * D, generator=torch.Generator().manual_seed(D), dtype=torch.float64)
    doc = torch.repeat_interleave(torch.arange(3), torch.tensor(lens)).expand(B, L)
    got = attention_reference(qkv, B, H, L, causal=True, kv_heads=Hkv, head_dim=D, key_start=doc_key_start(doc))
    got, x, t0 = got.view(B, L, -1), qkv.view(B, L, -1), 0
    for n in lens:
        piece = x[:, t0:t0 + n].reshape(B * n, -1)
        want = attention_reference(piece, B, H, n, causal=True, kv_heads=Hkv, head_dim=D).view(B, n, -1)
        assert torch.allclose(got[:, t0:t0 + n], want, rtol=0, atol=1e-12)
        t0 += n


@pytest.mark.parametrize("kw", [{}, dict(hidden=256, heads=2, kv_heads=1, head_dim=128)])
def test_packed_row_equals_its_documents(kw):
    """fp32 llama_tiny: logits of a packed row = each document as its own sequence with positions
    restarted at 0 (RoPE by row position changes no score); the loss is their token-weighted mean,
    n - 1 targets a document: nothing is scored across a boundary."""
    from kubeml_amd.models.llama import llama_tiny
    m = llama_tiny(**kw).eval()
    g = torch.Generator().manual_seed(5)
    docs = [torch.randint(1, 1000, (n,), generator=g) for n in (9, 1, 14, 6)]
    ids, mask, doc = pack_documents(docs, 32)
    labels = ids.masked_fill(mask == 0, -100)
    with torch.no_grad():
        logits, loss = m(ids, mask, doc_ids=doc), m(ids, mask, labels=labels, doc_ids=doc)
        t0, tot, cnt = 0, 0.0, 0
        for d in docs:
            n = d.numel()
            assert torch.allclose(logits[t0:t0 + n], m(d[None]), rtol=1e-4, atol=1e-4)
            if n > 1:
                tot, cnt = tot + m(d[None], labels=d[None]).item() * (n - 1), cnt + n - 1
            t0 += n
        assert ids.shape == (1, 32) and abs(loss.item() - tot / cnt) < 1e-4
        # without doc_ids the same row scores across the boundaries and lets documents see each other
        assert abs(m(ids, mask, labels=labels).item() - tot / cnt) > 1e-3
