"""GPU: K9L (csrc/k_attn.hip, core.vit_attention_long), the ViT attention for long sequences, and the high-resolution
towers it serves.

  * against the float64 math definition at T from 257 to the documented maximum (K9's error formula);
  * bit for bit K9's result wherever K9 runs (T <= 256), and independent of the batch it sits in, a batch whose qkv
    passes 2^31 bytes included;
  * the argument checks;
  * 1024 x 1024 and 1520 x 912 towers against the same towers on PyTorch's SDPA, and the drop-in driver at Mammo-CLIP's
    1520 x 912 input checked against the oracle.
"""
import glob
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core as c
    return c


def _attention(qkv, H, dtype, budget=1 << 26):
    """softmax(q k^T / 8) v in `dtype`, per query chunk: at most `budget` scores at a time (512 MB in float64)."""
    B, T, _ = qkv.shape
    q, k, v = qkv.to(dtype).view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)      # [B, H, T, 64] each
    out = torch.empty(B, H, T, 64, dtype=dtype, device=qkv.device)
    chunk = max(1, budget // (B * H * T))
    kt = k.transpose(-1, -2)
    for i in range(0, T, chunk):
        out[:, :, i:i + chunk] = torch.softmax(q[:, :, i:i + chunk] @ kt / 8.0, dim=-1) @ v
    return out.transpose(1, 2).reshape(B, T, H * 64)


@pytest.mark.parametrize("T", [257, 300, 512, 513, 1025, 4097, 5416, 32768])
@pytest.mark.parametrize("H", [1, 12])
def test_long_attention_matches_float64(core, dev, T, H):
    """Against the float64 definition, with K9's bound: 3e-6 * max(1, |ref|) + 3 x the fp32 bmm-softmax-bmm chain's own
    error on the same inputs (it grows with the score magnitude).  Partial and full last key tiles and query blocks,
    one query past a block (513, 4 097 = 1024 x 1024 at patch 16), 5 416 (1520 x 912) and the limit."""
    assert T <= core.VIT_ATTENTION_LONG_MAX_T
    B = 2 if T <= 1025 else 1
    g = torch.Generator(device=dev).manual_seed(T * 100 + H)
    for scale in (1.0, 6.0):
        qkv = torch.randn(B, T, 3 * H * 64, device=dev, generator=g) * scale
        out = core.vit_attention_long(qkv, H)
        ref = _attention(qkv, H, torch.float64)
        err = (out.double() - ref).abs().max().item()
        err32 = (_attention(qkv, H, torch.float32).double() - ref).abs().max().item()
        assert err <= 3e-6 * max(1.0, ref.abs().max().item()) + 3 * err32, (T, H, scale, err, err32)
        del ref


@pytest.mark.parametrize("T", [1, 5, 32, 33, 197, 256])
def test_long_attention_is_k9_bit_for_bit(core, dev, T):
    """Where K9 runs, the long form gives its bits: a query's arithmetic is the same, in the same order."""
    g = torch.Generator(device=dev).manual_seed(7 + T)
    for B, H, scale in ((3, 12, 1.0), (2, 1, 6.0)):
        qkv = torch.randn(B, T, 3 * H * 64, device=dev, generator=g) * scale
        assert torch.equal(core.vit_attention_long(qkv, H), core.vit_attention(qkv, H)), (T, B, H)


def test_long_attention_batch_invariant(core, dev):
    """Every image of a batched call equals the call on that image alone (T = 4 097: 17 query blocks, the last one
    query long); `out=` writes the same bits."""
    B, T, H = 3, 4097, 12
    g = torch.Generator(device=dev).manual_seed(11)
    qkv = torch.randn(B, T, 3 * H * 64, device=dev, generator=g) * 3
    out = core.vit_attention_long(qkv, H)
    for i in range(B):
        assert torch.equal(out[i:i + 1], core.vit_attention_long(qkv[i:i + 1].clone(), H)), i
    out2 = torch.full_like(out, float("nan"))
    assert core.vit_attention_long(qkv, H, out=out2) is out2
    assert torch.equal(out, out2)


def test_long_attention_past_2g_bytes(core, dev):
    """A batch whose qkv passes 2^31 bytes (60 images of 4 097 tokens x 12 heads: 2.26 GB): the first and the last
    image equal the calls on those images alone (each image's base address is 64-bit, its offsets stay 32-bit)."""
    B, T, H = 60, 4097, 12
    W = 3 * H * 64
    assert B * T * W * 4 > 2 ** 31
    g = torch.Generator(device=dev).manual_seed(13)
    qkv = torch.zeros(B, T, W, device=dev)
    qkv[0].normal_(generator=g)
    qkv[-1].normal_(generator=g)
    qkv[-1] *= 4
    out = core.vit_attention_long(qkv, H)
    first, last = out[0:1].clone(), out[-1:].clone()
    zero = out[1:2].clone()
    del out
    torch.cuda.synchronize()
    assert torch.equal(last, core.vit_attention_long(qkv[-1:].clone(), H))
    assert torch.equal(first, core.vit_attention_long(qkv[0:1].clone(), H))
    assert torch.equal(zero, torch.zeros_like(zero))            # v = 0 everywhere in image 1


def test_long_attention_refuses(core, dev, mcd):
    L = mcd._lib.load()
    buf = torch.zeros(1, 64, 3 * 64, device=dev)
    out = torch.zeros(1, 64, 64, device=dev)
    # T = 0 (through the C entry; the wrapper passes a zero-length tensor on as well)
    assert L.mcd_vit_attention_long(buf.data_ptr(), 1, 0, 1, out.data_ptr(), None) == -1
    assert "bad shape" in L.mcd_last_error().decode()
    with pytest.raises(mcd._lib.McdError) as e:
        core.vit_attention_long(torch.zeros(1, 0, 3 * 64, device=dev), 1)
    assert e.value.code == -1
    # a last dimension that is not 3 * heads * 64
    with pytest.raises(ValueError):
        core.vit_attention_long(torch.zeros(1, 300, 3 * 64 + 4, device=dev), 1)
    with pytest.raises(ValueError):
        core.vit_attention_long(torch.zeros(1, 300, 3 * 2 * 64, device=dev), 1)
    # a pointer that is not 16-byte aligned (a contiguous view 4 bytes into a buffer)
    flat = torch.zeros(300 * 3 * 64 + 1, device=dev)
    with pytest.raises(mcd._lib.McdError) as e:
        core.vit_attention_long(flat[1:].view(1, 300, 3 * 64), 1)
    assert e.value.code == -1 and "aligned" in str(e.value)
    # past the documented limit
    Tmax = core.VIT_ATTENTION_LONG_MAX_T
    with pytest.raises(mcd._lib.McdError) as e:
        core.vit_attention_long(torch.zeros(1, Tmax + 1, 3 * 64, device=dev), 1)
    assert e.value.code == mcd._lib.MCD_E_UNSUPPORTED and str(Tmax) in str(e.value)
    # one image's qkv block past 2^31 bytes (checked before any memory is touched: the pointer is never read)
    assert L.mcd_vit_attention_long(buf.data_ptr(), 1, Tmax, 100, out.data_ptr(), None) == mcd._lib.MCD_E_UNSUPPORTED
    assert "2^31" in L.mcd_last_error().decode()


@pytest.mark.parametrize("size", [1024, (1520, 912)])
def test_high_resolution_tower_on_the_long_kernel(mcd, dev, monkeypatch, size):
    """ViT towers at configs[4]'s 1024 x 1024 (4 097 tokens) and Mammo-CLIP's 1520 x 912 (5 416 tokens) with the HIP
    attention against the same towers on PyTorch's SDPA, within the 224 tower test's 1e-4; every attention call went
    to K9L.  The fused patch embedding (K11 + one GEMM) of the non-square input against the convolution."""
    from mammo_clip_dissect_amd import core
    from mammo_clip_dissect_amd.concept_vit import data_utils
    calls = []
    real = core.vit_attention_long

    def counting(qkv, heads, out=None):
        calls.append(tuple(qkv.shape))
        return real(qkv, heads, out)

    monkeypatch.setattr(core, "vit_attention_long", counting)
    torch.manual_seed(0)
    tower = data_utils.ViTTower(image_size=size, depth=2).to(dev).eval()
    for p in tower.parameters():
        torch.nn.init.normal_(p, std=0.05)
    Hh, Ww = data_utils.image_hw(size)
    T = 1 + (Hh // 16) * (Ww // 16)
    assert tower.pos_embed.shape[1] == T
    x = torch.randn(2, 3, Hh, Ww, device=dev)
    with torch.no_grad():
        assert data_utils.HIP_ATTENTION
        a = tower(x)
        assert calls == [(2, T, 3 * 768)] * 2
        data_utils.HIP_ATTENTION = False
        try:
            b = tower(x)
        finally:
            data_utils.HIP_ATTENTION = True
        assert len(calls) == 2
        e = tower.embed(x)
        c = tower.patch_embed(x).flatten(2).transpose(1, 2)
        c = torch.cat([tower.cls_token.expand(2, -1, -1), c], dim=1) + tower.pos_embed
    assert a.shape == (2, T, 768)
    assert (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item())
    assert (e - c).abs().max().item() <= 1e-4 * max(1.0, c.abs().max().item())


def test_driver_at_mammo_clip_resolution(dev, oracle, tmp_path):
    """describe_broad_neurons at Mammo-CLIP's own 1520 x 912 input ('breastclip_vit_1520x912', probes
    'synthetic_48_1520x912'), the CSV checked against the oracle on the run's own cache files."""
    from test_gpu_pipeline import _check_csv_against_oracle
    from mammo_clip_dissect_amd.concept_vit import describe_broad_neurons as drv
    layers = ["image_encoder.encoder.layer[0]", "image_encoder.encoder.layer[5]", "image_encoder.encoder.layer[11]"]
    act, res = str(tmp_path / "acts"), str(tmp_path / "results")
    out = drv.main(["--target_model", "breastclip_vit_1520x912", "--target_layers", ",".join(layers), "--d_probe",
                    "synthetic_48_1520x912", "--concept_set", CONCEPTS, "--batch_size", "8", "--device", str(dev),
                    "--activation_dir", act, "--result_dir", res, "--top_k", "20"])
    csvs = glob.glob(os.path.join(out, "*.csv"))
    assert len(csvs) == 1
    with open(CONCEPTS) as f:
        words = f.read().split("\n")
    _check_csv_against_oracle(csvs[0], act + "/**/*.pt", layers, oracle, "og", 20, words)
