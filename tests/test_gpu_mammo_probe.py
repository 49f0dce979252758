"""GPU: K23 (mcd_image_minmax_normalize, csrc/k_image.hip) and the mammogram probe sets' device route, bit for bit against
what the reference's own dataset classes return (the goldens of tests/golden/make_golden_mammo.py), and the Mammo-CLIP
driver from a vindr tree of PNG files: device route == host route, byte for byte."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mammo_recipe as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")
GUARD = 64              # guard elements in front of and behind every buffer of a C-ABI call
FILL = -777.25          # what the output buffer holds before the call
WS_FILL = -123456       # what the workspace and its guards hold before the call
MODES = {"minmax": 0, "raw": 1}


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call_k23(mcd, dev, src_np, mode, mean, std, dst_gap=0, guard_byte=0, shift=0):
    """One mcd_image_minmax_normalize call through ctypes on guarded buffers; the source starts `shift` bytes behind a
    64-byte boundary.  Returns (rc, the whole output buffer on the CPU, the image stride in elements, the workspace with
    its guards on the CPU, the workspace's int32 count)."""
    n, H, W = src_np.shape[:3]
    channels = 3 if src_np.ndim == 4 else 1
    lead = GUARD + shift
    sbuf = torch.full((lead + src_np.size + GUARD,), guard_byte, dtype=torch.uint8)
    sbuf[lead:lead + src_np.size] = torch.from_numpy(np.array(src_np)).reshape(-1)      # a copy: the shared input stays read-only
    sbuf = sbuf.to(dev)
    per = 3 * H * W
    dst_img = per + dst_gap
    obuf = torch.full((GUARD + n * dst_img + GUARD,), FILL, dtype=torch.float32, device=dev)
    L = mcd._lib.load()
    ws_bytes = L.mcd_image_minmax_workspace(n, H, W, channels)
    assert ws_bytes % 8 == 0 and ws_bytes > 0
    wbuf = torch.full((GUARD + ws_bytes // 4 + GUARD,), WS_FILL, dtype=torch.int32, device=dev)
    rc = L.mcd_image_minmax_normalize(_ptr(sbuf[lead:]), n, H, W, channels, MODES[mode], mean, std, _ptr(obuf[GUARD:]),
                                      dst_img, _ptr(wbuf[GUARD:]), ws_bytes, None)
    torch.cuda.synchronize()
    return rc, obuf.cpu(), dst_img, wbuf.cpu(), ws_bytes // 4


@pytest.mark.parametrize("name", R.case_names())
def test_k23_equals_the_reference_bit_for_bit(mcd, core, dev, name):
    """Every golden case through the C ABI: the fp32 bits of the reference's __getitem__ (sha256 as well for the workload
    shape); the guard elements around the output and the gap between its images keep their fill; guard bytes of 0 and of
    255 around the source give the same bits (a reduction that reads one byte past an image would move its min or max),
    at an aligned source and at one 3 bytes off (the reduction's head, the scalar path); the workspace's guards keep
    their fill and its pairs are every chunk's min and max."""
    c = R.case(name)
    src = R.case_input(c)
    n, H, W = src.shape[:3]
    per = 3 * H * W
    for guard_byte, shift in ((0, 0), (255, 0), (0, 3), (255, 3)):
        rc, buf, dst_img, ws, ws_n = _call_k23(mcd, dev, src, c["mode"], c["mean"], c["std"], c["dst_gap"], guard_byte, shift)
        assert rc == 0, mcd._lib.load().mcd_last_error()
        body = buf[GUARD:GUARD + n * dst_img].view(n, dst_img)
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n * dst_img:] == FILL).all())
        assert bool((body[:, per:] == FILL).all())
        R.check_against_golden(c, body[:, :per].reshape(n, 3, H, W).contiguous().numpy())
        assert bool((ws[:GUARD] == WS_FILL).all()) and bool((ws[GUARD + ws_n:] == WS_FILL).all())
        pairs = ws[GUARD:GUARD + ws_n].view(n, -1, 2).numpy()
        if c["mode"] == "raw":
            assert bool((pairs == WS_FILL).all())                         # RAW does not touch the workspace
        else:
            flat = src.reshape(n, -1)
            chunk = core.IMAGE_MINMAX_CHUNK                               # doubled until at most 256 chunks cover an image
            while -(-flat.shape[1] // chunk) > 256:
                chunk *= 2
            assert pairs.shape[1] == -(-flat.shape[1] // chunk)
            for k in range(pairs.shape[1]):
                piece = flat[:, k * chunk:(k + 1) * chunk]
                assert np.array_equal(pairs[:, k, 0], piece.min(axis=1)) and np.array_equal(pairs[:, k, 1], piece.max(axis=1))


def test_k23_chunk_doubles_past_256_chunks(mcd, core, dev):
    """An image of 256 chunks + 1 byte: the chunk doubles (129 pairs); the only 255 is the last byte."""
    size = 256 * core.IMAGE_MINMAX_CHUNK + 1
    src = np.random.RandomState(3).randint(4, 200, (1, 1, size)).astype(np.uint8)
    src[0, 0, -1] = 255
    src[0, 0, 12345] = 1
    c = dict(mode="minmax", mean=0.25, std=0.5)
    rc, buf, dst_img, ws, ws_n = _call_k23(mcd, dev, src, "minmax", 0.25, 0.5)
    assert rc == 0 and ws_n == 2 * 129
    got = buf[GUARD:GUARD + 3 * size].view(1, 3, 1, size).numpy()
    assert np.array_equal(got.view(np.uint32), R.numpy_apply(src, c).view(np.uint32))


def test_k23_argument_contract(mcd, core, dev):
    """Every refusal of the entry, each leaving dst untouched."""
    L = mcd._lib.load()
    E_ARG, E_WS, E_UNSUPPORTED = mcd._lib.MCD_E_ARG, mcd._lib.MCD_E_WORKSPACE, mcd._lib.MCD_E_UNSUPPORTED
    H, W = 8, 12
    x = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, device=dev)
    out = torch.full((2 * 3 * H * W + 16,), FILL, dtype=torch.float32, device=dev)
    ws = torch.zeros((64,), dtype=torch.int32, device=dev)

    def call(src=x, n=2, H=H, W=W, channels=3, mode=0, dst=out, dst_img=3 * H * W, ws=ws, ws_bytes=256):
        return L.mcd_image_minmax_normalize(_ptr(src), n, H, W, channels, mode, 0.3, 0.25, _ptr(dst), dst_img, _ptr(ws),
                                            ws_bytes, None)

    def refused(code, **kw):
        rc = call(**kw)
        torch.cuda.synchronize()
        return rc == code and bool((out == FILL).all())
    assert refused(E_ARG, src=None) and refused(E_ARG, dst=None)
    assert refused(E_ARG, channels=2) and refused(E_ARG, channels=4) and refused(E_ARG, channels=0)
    assert refused(E_ARG, mode=2) and refused(E_ARG, mode=-1)
    assert refused(E_ARG, H=0) and refused(E_ARG, W=0) and refused(E_ARG, n=-1)
    assert refused(E_ARG, dst_img=3 * H * W - 1)
    assert refused(E_ARG, src=out.view(torch.uint8))                                   # src overlaps dst
    assert refused(E_ARG, ws=out[8:].view(torch.int32))                                # ws overlaps dst
    assert refused(E_ARG, ws=None)                                                     # MINMAX needs its workspace
    assert refused(E_WS, ws_bytes=8) and refused(E_WS, ws_bytes=0)
    assert L.mcd_image_minmax_workspace(2, H, W, 3) == 16
    assert refused(E_UNSUPPORTED, n=65536, ws_bytes=1 << 30)
    assert refused(E_UNSUPPORTED, H=1 << 16, W=1 << 15, channels=1, dst_img=3 << 31)   # the source reaches 2^31 bytes
    assert refused(E_UNSUPPORTED, H=1 << 14, W=1 << 14, channels=1, dst_img=3 << 28)   # the output (3 GiB) does
    assert b"2^31" in L.mcd_last_error()
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # RAW ignores mean, std and the workspace; then the accepted MINMAX call
    assert call(mode=1, ws=None, ws_bytes=0) == 0
    torch.cuda.synchronize()
    got = out[:2 * 3 * H * W].view(2, 3, H, W)
    assert torch.equal(got, x.permute(0, 3, 1, 2).float()) and bool((out[2 * 3 * H * W:] == FILL).all())
    assert call(ws_bytes=16) == 0
    torch.cuda.synchronize()
    c = dict(mode="minmax", mean=0.3, std=0.25)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), R.numpy_apply(x.cpu().numpy(), c).view(np.uint32))


def test_image_minmax_normalize_writes_into_a_batch_slice(core, dev):
    c = R.case("batch3")
    src = torch.from_numpy(R.case_input(c)).to(dev)
    batch = torch.full((6, 3, 16, 16), FILL, dtype=torch.float32, device=dev)
    core.image_minmax_normalize(src, c["mean"], c["std"], out=batch[2:5])
    assert bool((batch[:2] == FILL).all()) and bool((batch[5] == FILL).all())
    R.check_against_golden(c, batch[2:5].cpu().numpy())
    # an image's bits depend neither on its batch nor on its place in it
    alone = core.image_minmax_normalize(src[1:2].contiguous(), c["mean"], c["std"])
    assert torch.equal(alone[0].view(torch.int32), batch[3].view(torch.int32))
    rgb = R.case("rgb_channels")
    R.check_against_golden(rgb, core.image_minmax_normalize(torch.from_numpy(R.case_input(rgb)).to(dev), rgb["mean"],
                                                            rgb["std"]).cpu().numpy())
    raw = R.case("csaw_raw")
    R.check_against_golden(raw, core.image_minmax_normalize(torch.from_numpy(R.case_input(raw)).to(dev), 0.0, 1.0,
                                                            mode="raw").cpu().numpy())
    with pytest.raises(ValueError, match="out must be"):
        core.image_minmax_normalize(src, c["mean"], c["std"], out=batch[:3, :, :, :15])
    with pytest.raises(TypeError, match="contiguous uint8"):
        core.image_minmax_normalize(src.float(), c["mean"], c["std"])
    with pytest.raises(ValueError, match="mode"):
        core.image_minmax_normalize(src, c["mean"], c["std"], mode="zscore")


def _png_tree(tmp_path, n, H, W, seed, rgb_every=0):
    """n PNGs (mode L; every rgb_every-th RGB) under the reference's vindr layout + CSV, and a csaw CSV over the grey
    ones.  Images have different value ranges, so every one has its own table."""
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(seed)
    vindr, csaw = ["patient_id,image_id,split,Mass"], ["anon_filename,Cancer_visible,split"]
    for i in range(n):
        lo = int(rs.randint(0, 60))
        hi = int(rs.randint(lo + 40, 256))
        rgb = rgb_every and i % rgb_every == rgb_every - 1
        a = rs.randint(lo, hi + 1, (H, W, 3) if rgb else (H, W)).astype(np.uint8)
        d = tmp_path / "VinDR_MammoCLIP" / "images_png" / ("%03d" % (i // 2))
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray(a, "RGB" if rgb else "L").save(str(d / ("im%02d.png" % i)))
        vindr.append("%03d,im%02d%s,test,%d" % (i // 2, i, ".png" if i % 3 == 0 else "", i % 2))
        if not rgb:
            csaw.append("im%02d.dcm,%d,test" % (i, i % 2))
            os.symlink(str(d / ("im%02d.png" % i)), str(tmp_path / ("im%02d.png" % i)))
    vindr.insert(3, "999,skipped,training,0")
    (tmp_path / "VinDR-data").mkdir()
    (tmp_path / "VinDR-data" / "vindr_detection_v1_folds.csv").write_text("\n".join(vindr) + "\n")
    (tmp_path / "csaw.csv").write_text("\n".join(csaw) + "\n")


def test_device_route_equals_host_route(du, dev, tmp_path, monkeypatch):
    """ImageFileProbe on 12 PNG files of a vindr tree, batches of 5 (the last one short; every fourth file RGB, so a batch
    holds runs of both channel counts): device_batches == the stacked host items, bit for bit, for vindr and for csaw."""
    monkeypatch.setattr(du, "DATASET_ROOTS", {})
    monkeypatch.delenv("MCD_DATASETS", raising=False)
    _png_tree(tmp_path, 12, 48, 40, seed=7, rgb_every=4)
    du.register_dataset("vindr", root=str(tmp_path))
    du.register_dataset("csaw", root=str(tmp_path), csv="csaw.csv", path=str(tmp_path))
    for name, n in (("vindr", 12), ("csaw", 9)):
        host, ds = du.get_data(name), du.get_data(name, device=dev)
        assert len(host) == n and len(ds) == n and host.device is None and ds.device == dev
        want = torch.stack([host[i][0] for i in range(n)])
        batches = list(ds.device_batches(5))
        assert [b.shape[0] for b in batches] == ([5, 5, 2] if n == 12 else [5, 4])
        got = torch.cat(batches).cpu()
        assert got.dtype == torch.float32 and got.shape == (n, 3, 48, 40)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(ds.sample().cpu(), want[:1])


def test_broad_driver_on_vindr_device_route_equals_host_route(du, dev, tmp_path, monkeypatch):
    """describe_broad_neurons --d_probe vindr (the drivers' default probe set) on 24 PNG files of 96 x 64, the random-weight
    breastclip target, two layers: the device route (K23) and MCD_PROBE_ON_HOST=1 (numpy + DataLoader) write
    byte-identical descriptions.csv."""
    from mammo_clip_dissect_amd.concept_vit import describe_broad_neurons as drv
    monkeypatch.setattr(du, "DATASET_ROOTS", {})
    monkeypatch.delenv("MCD_DATASETS", raising=False)
    monkeypatch.delenv("MCD_PROBE_ON_HOST", raising=False)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    _png_tree(tmp_path, 24, 96, 64, seed=11)
    du.register_dataset("vindr", root=str(tmp_path))

    def run(tag):
        act, res = str(tmp_path / ("acts_" + tag)), str(tmp_path / ("results_" + tag))
        out = drv.main(["--target_model", "breastclip", "--target_layers", "image_encoder._blocks[0],image_encoder._blocks[20]",
                        "--d_probe", "vindr", "--concept_set", CONCEPTS, "--batch_size", "10", "--top_k", "10",
                        "--device", str(dev), "--activation_dir", act, "--result_dir", res])
        csvs = [f for f in os.listdir(out) if f.endswith(".csv")]
        assert len(csvs) == 1
        return open(os.path.join(out, csvs[0]), "rb").read()
    csv_dev = run("device")
    monkeypatch.setenv("MCD_PROBE_ON_HOST", "1")
    csv_host = run("host")
    assert csv_dev == csv_host and len(csv_dev) > 0
