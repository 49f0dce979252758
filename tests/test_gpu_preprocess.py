"""GPU: K22 (mcd_image_preprocess, csrc/k_image.hip) and the file probe sets' device route, bit for bit against what PIL +
torch compute (the goldens of tests/golden/make_golden_preprocess.py), and the vanilla CLIP-Dissect driver from a folder
of PNG files: device route == host route, byte for byte."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import preprocess_recipe as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")
GUARD = 64              # guard elements in front of and behind every buffer of a C-ABI call
FILL = -777.25          # what the output buffer holds before the call


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


def _call_k22(mcd, dev, src_np, plan, lut, dst_gap, guard_byte, tabs=None):
    """One mcd_image_preprocess call through ctypes on guarded buffers.  Returns (rc, the whole output buffer on the
    CPU, the image stride in elements)."""
    n, H, W = src_np.shape[:3]
    sbuf = torch.full((GUARD + src_np.size + GUARD,), guard_byte, dtype=torch.uint8)
    sbuf[GUARD:GUARD + src_np.size] = torch.from_numpy(np.ascontiguousarray(src_np)).reshape(-1)
    sbuf = sbuf.to(dev)
    src = sbuf[GUARD:]
    per = 3 * plan.OH * plan.OW
    dst_img = per + dst_gap
    obuf = torch.full((GUARD + n * dst_img + GUARD,), FILL, dtype=torch.float32, device=dev)
    xtab, ytab = tabs if tabs is not None else (plan.xtab, plan.ytab)
    xtab = None if xtab is None else xtab.to(dev)
    ytab = None if ytab is None else ytab.to(dev)
    kx, ky = (0 if t is None else t.shape[1] - 2 for t in (xtab, ytab))
    L = mcd._lib.load()
    rc = L.mcd_image_preprocess(_ptr(src), n, H, W, _ptr(xtab), kx, plan.RW, _ptr(ytab), ky, plan.RH, plan.top, plan.left,
                                plan.OH, plan.OW, _ptr(lut), _ptr(obuf[GUARD:]), dst_img, None)
    torch.cuda.synchronize()
    return rc, obuf.cpu(), dst_img


@pytest.mark.parametrize("name", R.case_names())
def test_k22_equals_pil_bit_for_bit(mcd, core, dev, name):
    """Every golden case through the C ABI: the fp32 bits PIL + torch give (sha256 as well for the workload shapes); the
    guard elements around the output and the gap between its images keep their fill; guard bytes of 0 or of 255 around
    the input give the same result (nothing outside the images is read into it)."""
    c = R.case(name)
    pre = R.spec_of(core, c)
    src = R.case_input(c)
    n = src.shape[0]
    plan = pre.plan(src.shape[1], src.shape[2])
    lut = pre.lut().to(dev)
    per = 3 * plan.OH * plan.OW
    results = []
    for guard_byte in (0, 255):
        rc, buf, dst_img = _call_k22(mcd, dev, src, plan, lut, c["dst_gap"], guard_byte)
        assert rc == 0, mcd._lib.load().mcd_last_error()
        body = buf[GUARD:GUARD + n * dst_img].view(n, dst_img)
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n * dst_img:] == FILL).all())
        assert bool((body[:, per:] == FILL).all())
        results.append(body[:, :per].reshape(n, 3, plan.OH, plan.OW).contiguous())
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32))
    R.check_against_golden(c, results[0].numpy())


def test_k22_tap_cap_and_argument_errors(mcd, core, dev):
    """More coefficients per row than the kernel takes: MCD_E_UNSUPPORTED and an untouched output.  Aliasing, a crop
    window outside the resized image and a NULL table on a resized axis are MCD_E_ARG."""
    L = mcd._lib.load()
    E_ARG, E_UNSUPPORTED = mcd._lib.MCD_E_ARG, mcd._lib.MCD_E_UNSUPPORTED
    assert core.IMAGE_MAX_TAPS == 128
    pre = core.Preprocess("bilinear", (4, 4))
    src = np.random.RandomState(0).randint(0, 256, (1, 4 * 70, 4, 3)).astype(np.uint8)        # ratio 70: 141 vertical taps
    plan = pre.plan(280, 4)
    assert plan.taps[1] > core.IMAGE_MAX_TAPS and not plan.device_ok
    lut = pre.lut().to(dev)
    rc, buf, _ = _call_k22(mcd, dev, src, plan, lut, 0, 0)
    assert rc == E_UNSUPPORTED and b"taps" in L.mcd_last_error() and bool((buf == FILL).all())
    with pytest.raises(core.McdError) as e:
        core.image_preprocess(torch.from_numpy(src).to(dev), pre)
    assert e.value.code == E_UNSUPPORTED
    # exactly at the cap: a table padded to 128 columns is the same picture
    ok = core.Preprocess("bilinear", (4, 4)).plan(40, 4)
    small = src[:, :40].copy()
    padded = torch.zeros((4, 2 + 128), dtype=torch.int32)
    padded[:, :ok.ytab.shape[1]] = ok.ytab
    rc, want, _ = _call_k22(mcd, dev, small, ok, lut, 0, 0)
    rc2, got, _ = _call_k22(mcd, dev, small, ok, lut, 0, 0, tabs=(None, padded))
    assert rc == 0 and rc2 == 0 and torch.equal(want, got)

    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    out = torch.full((3 * 8 * 8,), FILL, dtype=torch.float32, device=dev)

    def call(src_t, dst_t, RW=8, RH=8, top=0, left=0, OH=8, OW=8, lut_t=lut):
        return L.mcd_image_preprocess(_ptr(src_t), 1, 8, 8, None, 0, RW, None, 0, RH, top, left, OH, OW, _ptr(lut_t),
                                      _ptr(dst_t), 3 * OH * OW, None)
    assert call(x, out) == 0
    assert call(x, out, top=1) == E_ARG                       # the window leaves the image
    assert call(x, out, RW=7, OW=7) == E_ARG                  # a resized axis without a table
    assert call(x, out, lut_t=out) == E_ARG                   # lut aliases dst
    assert call(out.view(torch.uint8), out) == E_ARG          # src aliases dst
    assert call(None, out) == E_ARG
    torch.cuda.synchronize()


def _route_probe(du, core, dev, two_views=True):
    z, meta = R.goldens()
    views = {v: R.spec_of(core, s) for v, s in meta["route"]["views"].items()}
    samples = [("route_in_%d" % i, 0) for i in range(meta["route"]["n"])]
    return du.ImageFileProbe(samples, views["a"], views["b"] if two_views else None, decode=lambda key: z[key],
                             device=dev), z


def test_device_route_equals_host_route(du, core, dev):
    """ImageFileProbe.device_batches on arrays served from the goldens (no PIL on this route): seven images of four
    source sizes at batch 5 -- runs of 1, 1 and 3 same-size images in the first batch, a tail of 2 -- two views from one
    upload: the bits of the host route's tensors (PIL + torch, stored in the npz)."""
    ds, z = _route_probe(du, core, dev)
    batches = list(ds.device_batches(5))
    assert [tuple(b[0].shape) for b in batches] == [(5, 3, 12, 12), (2, 3, 12, 12)]
    for v, key in ((0, "route_out_a"), (1, "route_out_b")):
        got = torch.cat([b[v] for b in batches]).cpu()
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), torch.from_numpy(z[key]).view(torch.int32))
    assert torch.equal(ds.sample().cpu(), torch.from_numpy(z["route_out_a"][:1]))
    one, _ = _route_probe(du, core, dev, two_views=False)            # one view: plain tensors, not pairs
    got = torch.cat(list(one.device_batches(3))).cpu()
    assert torch.equal(got, torch.from_numpy(z["route_out_a"]))
    shard = du.ImageFileProbe(ds.samples, ds.preprocess, decode=ds.decode, lo=3, hi=6, device=dev)
    assert torch.equal(torch.cat(list(shard.device_batches(2))).cpu(), torch.from_numpy(z["route_out_a"][3:6]))


def test_image_preprocess_writes_into_a_batch_slice(core, dev):
    c = R.case("c7_three")
    pre = R.spec_of(core, c)
    src = torch.from_numpy(R.case_input(c)).to(dev)
    batch = torch.full((5, 3, 12, 12), FILL, dtype=torch.float32, device=dev)
    core.image_preprocess(src, pre, out=batch[1:4])
    assert bool((batch[0] == FILL).all()) and bool((batch[4] == FILL).all())
    R.check_against_golden(c, batch[1:4].cpu().numpy())
    with pytest.raises(ValueError, match="out must be"):
        core.image_preprocess(src, pre, out=batch[:3, :, :, :11])


def test_driver_from_png_files_device_route_equals_host_route(du, dev, tmp_path, monkeypatch):
    """describe_clip_neurons on a class-folder tree of 128 PNG files (ResNet-18 target with the ImageNet transform, the
    dissector with CLIP's: two views of one decode): the device route (K22) and MCD_PROBE_ON_HOST=1 (PIL + torch +
    DataLoader) write byte-identical descriptions.csv and equal dissector embeddings."""
    Image = pytest.importorskip("PIL.Image")
    from mammo_clip_dissect_amd.concept_vit import describe_clip_neurons as drv
    root = tmp_path / "pngs"
    rs = np.random.RandomState(99)
    for i in range(128):
        d = root / ("class_%d" % (i % 4))
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray(rs.randint(0, 256, (40, 56, 3)).astype(np.uint8), "RGB").save(str(d / ("img_%03d.png" % i)))
    monkeypatch.setattr(du, "DATASET_KINDS", dict(du.DATASET_KINDS))
    monkeypatch.setattr(du, "DATASET_ROOTS", {})
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    du.register_dataset("png_probe", path=str(root), kind="folder", default_preprocess="imagenet")
    ds = du.get_data("png_probe", "imagenet", dev, clip_preprocess="clip")
    assert len(ds) == 128 and len(ds.views) == 2 and os.path.basename(ds.samples[1][0]) == "img_004.png"

    def run(tag):
        act, res = str(tmp_path / ("acts_" + tag)), str(tmp_path / ("results_" + tag))
        out = drv.main(["--target_model", "resnet18", "--target_layers", "layer3,layer4", "--d_probe", "png_probe",
                        "--concept_set", CONCEPTS, "--batch_size", "48", "--device", str(dev), "--activation_dir", act,
                        "--result_dir", res])
        emb = [f for f in glob.glob(os.path.join(act, "**", "*.pt"), recursive=True)
               if os.path.basename(f).startswith("png_probe_ViT")]
        assert len(emb) == 1
        return open(os.path.join(out, "descriptions.csv"), "rb").read(), torch.load(emb[0], weights_only=True)
    csv_dev, emb_dev = run("device")
    monkeypatch.setenv("MCD_PROBE_ON_HOST", "1")
    csv_host, emb_host = run("host")
    assert csv_dev == csv_host and len(csv_dev) > 0
    assert emb_dev.shape[0] == 128 and torch.equal(emb_dev, emb_host)
