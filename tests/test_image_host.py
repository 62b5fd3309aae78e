"""The image pipeline's host side (no GPU): the restatement against the PIL-minted golden and PIL itself, the size and crop
rules, the tables and descriptors transvae.image_io hands to the kernel, the uint8 collate, the PNG writer, the grid geometry
and the argument errors."""
import io
import json
import os

import numpy as np
import pytest
import torch

import image_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep_pil.npz")


def load_golden():
    g = np.load(GOLDEN)
    cases = json.loads(bytes(g["cases"]).decode())
    return g, cases


def case_kw(c):
    return dict(resize=tuple(c["resize"])) if "resize" in c else dict(res=c["res"])


def test_golden_is_from_pillow_and_small():
    g, cases = load_golden()
    assert bytes(g["pillow_version"]).decode().split(".")[0].isdigit()
    assert os.path.getsize(GOLDEN) < 300 * 1024
    assert len(cases) == 12 and max(g["in_" + c["name"]].size for c in cases) == 128 * 192 * 3


def test_restatement_equals_golden():
    g, cases = load_golden()
    for c in cases:
        out = R.prep_uint8(g["in_" + c["name"]], **case_kw(c))
        assert out.dtype == np.uint8 and np.array_equal(out, g["out_" + c["name"]]), c["name"]


def test_restatement_equals_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for h, w, oh, ow in [(37, 53, 16, 22), (53, 37, 22, 16), (17, 40, 32, 75), (33, 33, 64, 64), (31, 77, 48, 119), (32, 48, 32, 24),
                         (32, 48, 16, 48), (128, 192, 16, 24), (100, 333, 64, 213)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(R.pil_resize(img, oh, ow), ref), (h, w, oh, ow)


def test_size_and_crop_rules():
    from transvae.image_io import ImagePrep, center_crop_offsets, resize_size
    assert resize_size(500, 375, 256) == (341, 256) and resize_size(375, 500, 256) == (256, 341)
    assert resize_size(256, 300, 256) == (256, 300) and resize_size(300, 256, 256) == (300, 256)   # short == res: untouched
    assert resize_size(37, 53, 16) == (16, 22) and resize_size(100, 150, 72) == (72, 108)
    assert resize_size(720, 1280, 512) == (512, 910)
    # Python's round: half to even, both ways
    assert center_crop_offsets(16, 21, 16, 16) == (0, 2) and center_crop_offsets(16, 23, 16, 16) == (0, 4)
    assert center_crop_offsets(21, 16, 16, 16) == (2, 0) and center_crop_offsets(19, 17, 16, 16) == (2, 0)
    for h, w, res in [(37, 53, 16), (500, 375, 256), (16, 21, 16), (16, 23, 16), (100, 150, 72), (33, 33, 64)]:
        oh, ow = R.resize_size(h, w, res)
        assert ImagePrep(res).geometry(h, w) == (oh, ow, int(round((oh - res) / 2.0)), int(round((ow - res) / 2.0)))
    assert ImagePrep(resize=(16, 48)).geometry(32, 48) == (16, 48, 0, 0)
    # an image whose short side equals res is not resampled: no table on either axis
    d = ImagePrep(16).describe(torch.tensor([[0, 16, 21, 63, 3]]))[0]
    assert (d.xtab, d.ytab, d.crop_left, d.out_w) == (-1, -1, 2, 21)
    d = ImagePrep(resize=(32, 24)).describe(torch.tensor([[0, 32, 48, 144, 3]]))[0]
    assert d.xtab >= 0 and d.ytab == -1


def test_tables_equal_the_restatement_and_are_cached():
    from transvae.image_io import ImagePrep, bilinear_table
    for n_in, n_out, lo, n in [(53, 22, 3, 16), (37, 16, 0, 16), (40, 75, 21, 32), (192, 24, 4, 16), (150, 108, 18, 72)]:
        first, count, k = bilinear_table(n_in, n_out, lo, n)
        ref = list(R.coeffs(n_in, n_out))[lo:lo + n]
        assert k.dtype == np.int32 and k.shape[0] == n
        for i, (xmin, cnt, kk) in enumerate(ref):
            assert (first[i], count[i]) == (xmin, cnt) and list(k[i, :cnt]) == kk and not k[i, cnt:].any()
    prep = ImagePrep(16)
    table = torch.tensor([[0, 37, 53, 159, 3], [5883, 37, 53, 159, 3]])
    a = prep.describe(table)
    size = prep._coef.size
    b = prep.describe(table)
    assert prep._coef.size == size and (a[0].xtab, a[0].ytab) == (a[1].xtab, a[1].ytab) == (b[1].xtab, b[1].ytab)


def emulate_kernel(buf, descs, coef, res_h, res_w):
    """What tv_image_prep's kernel computes from the product's own descriptors and tables, in NumPy: uint8 [B, res_h, res_w, 3]."""
    out = np.zeros((len(descs), res_h, res_w, 3), np.uint8)
    for b, d in enumerate(descs):
        img = np.lib.stride_tricks.as_strided(buf[d.offset:], (d.in_h, d.in_w, 3), (d.row_stride, 3, 1)).astype(np.int64)
        if d.xtab >= 0:
            mn, cnt = coef[d.xtab:d.xtab + res_w], coef[d.xtab + res_w:d.xtab + 2 * res_w]
            k = coef[d.xtab + 2 * res_w:d.xtab + 2 * res_w + res_w * d.xk].reshape(res_w, d.xk).astype(np.int64)
            h = np.stack([np.clip(((1 << 21) + np.tensordot(k[x, :cnt[x]], img[:, mn[x]:mn[x] + cnt[x]], axes=(0, 1))) >> 22, 0, 255)
                          for x in range(res_w)], axis=1)
        else:
            h = img[:, d.crop_left:d.crop_left + res_w]
        if d.ytab >= 0:
            mn, cnt = coef[d.ytab:d.ytab + res_h], coef[d.ytab + res_h:d.ytab + 2 * res_h]
            k = coef[d.ytab + 2 * res_h:d.ytab + 2 * res_h + res_h * d.yk].reshape(res_h, d.yk).astype(np.int64)
            v = np.stack([np.clip(((1 << 21) + np.tensordot(k[y, :cnt[y]], h[mn[y]:mn[y] + cnt[y]], axes=(0, 0))) >> 22, 0, 255)
                          for y in range(res_h)], axis=0)
        else:
            v = h[d.crop_top:d.crop_top + res_h]
        out[b] = v
    return out


def test_descriptors_and_tables_reproduce_the_golden():
    """The product's cropped tables and descriptors, walked as the kernel walks them, give PIL's bytes -- packed tightly (odd
    starts) and with padded rows."""
    from transvae.image_io import ImagePrep, pack_uint8
    g, cases = load_golden()
    groups = {}
    for c in cases:
        groups.setdefault(json.dumps(case_kw(c)), []).append(c)
    for kw, cs in groups.items():
        kw = json.loads(kw)
        prep = ImagePrep(kw.get("res"), resize=kw.get("resize"))
        rh, rw = prep.output_size()
        for pack_kw in (dict(), dict(align=2, row_pad=5)):
            batch = pack_uint8([g["in_" + c["name"]] for c in cs], pin=False, **pack_kw)
            out = emulate_kernel(batch.data.numpy(), prep.describe(batch.table), prep._coef, rh, rw)
            for i, c in enumerate(cs):
                assert np.array_equal(out[i], g["out_" + c["name"]]), (c["name"], pack_kw)


def test_to_tensor_table_is_the_ieee_division():
    from transvae.image_io import ImagePrep
    v = np.arange(256, dtype=np.float32)
    unit = (v / np.float32(255.0)).astype(np.float32)
    assert np.array_equal(ImagePrep(8)._lut_host.numpy(), unit)
    assert np.array_equal(ImagePrep(8, range="signed")._lut_host.numpy(), unit * np.float32(2) - np.float32(1))
    assert np.any(unit != v * np.float32(1.0 / 255.0))         # the reciprocal multiply is NOT bit-equal
    assert torch.equal(R.to_tensor(np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2))[0].reshape(-1), torch.from_numpy(unit))


def test_collate_round_trips_offsets_and_strides():
    from transvae.image_io import UInt8Batch, collate_uint8, pack_uint8
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(5, 7, 3), (4, 3, 3), (9, 2, 3)]]
    batch = collate_uint8([(imgs[0], 4), (torch.from_numpy(imgs[1]), 5), (imgs[2][:, ::1], 6)], pin=False)
    assert isinstance(batch, UInt8Batch) and len(batch) == 3 and batch.data.dtype == torch.uint8 and batch.data.dim() == 1
    assert batch.table.tolist() == [[0, 5, 7, 21, 3], [105, 4, 3, 9, 3], [141, 9, 2, 6, 3]]
    assert batch.labels.tolist() == [4, 5, 6]
    for i, im in enumerate(imgs):
        assert np.array_equal(batch.image(i).numpy(), im)
    padded = pack_uint8(imgs, pin=False, align=4, row_pad=3)
    assert padded.table[:, 0].tolist() == [0, 120, 168] and padded.table[:, 3].tolist() == [24, 12, 9]
    for i, im in enumerate(imgs):
        assert np.array_equal(padded.image(i).numpy(), im)
    bare = collate_uint8(imgs, pin=False)
    assert bare.labels is None and bare.table.tolist() == batch.table.tolist()
    try:
        from PIL import Image
    except ImportError:
        return
    pil = collate_uint8([Image.fromarray(imgs[0], "RGB")], pin=False)
    assert np.array_equal(pil.image(0).numpy(), imgs[0])


def test_png_writer_round_trips(tmp_path):
    from transvae.image_io import encode_png, save_image
    rng = np.random.default_rng(5)
    for shape in [(1, 1, 3), (7, 13, 3), (64, 40, 3)]:
        rgb = rng.integers(0, 256, shape, dtype=np.uint8)
        data = encode_png(rgb)
        assert np.array_equal(R.decode_png(data), rgb)
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(io.BytesIO(data))
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), rgb)
    grid = torch.from_numpy(rng.integers(0, 256, (9, 11, 3), dtype=np.uint8))
    path = tmp_path / "grid.png"
    save_image(grid, path)                     # a uint8 grid is written as it is, from any device
    assert np.array_equal(R.decode_png(path.read_bytes()), grid.numpy())
    with pytest.raises(ValueError):
        encode_png(np.zeros((4, 4), np.uint8))


def test_grid_geometry_matches_the_restatement():
    from transvae.image_io import grid_geometry
    for B in (1, 2, 5, 8, 9):
        for nrow in (1, 4, 8):
            for padding in (0, 2, 3):
                Hg, Wg, xmaps, ymaps = grid_geometry(B, 6, 10, nrow, padding)
                assert (Hg, Wg) == R.grid_shape(B, 6, 10, nrow, padding)
                x = torch.arange(B * 3 * 6 * 10, dtype=torch.float32).reshape(B, 3, 6, 10)
                assert tuple(R.make_grid(x, nrow, padding, 0.5).shape) == (3, Hg, Wg)
    assert grid_geometry(1, 6, 10, 8, 2) == (6, 10, 1, 1)          # a batch of one: no border
    assert grid_geometry(8, 6, 10, 8, 0)[:2] == (6, 80)            # padding 0, one row: the plain batch row
    # placement and pad value
    x = torch.stack([torch.full((3, 2, 2), float(k + 1)) for k in range(3)])
    gr = R.make_grid(x, nrow=2, padding=1, pad_value=9.0)[0]
    assert gr.tolist() == [[9, 9, 9, 9, 9, 9, 9], [9, 1, 1, 9, 2, 2, 9], [9, 1, 1, 9, 2, 2, 9], [9, 9, 9, 9, 9, 9, 9],
                           [9, 3, 3, 9, 9, 9, 9], [9, 3, 3, 9, 9, 9, 9], [9, 9, 9, 9, 9, 9, 9]]
    q = R.quantise(torch.tensor([[[-0.1, 0.0, 0.5 / 255, 1.0, 1.2, float("nan")]]]).expand(3, 1, 6))
    assert q[0, :, 0].tolist() == [0, 0, 1, 255, 255, 0]


def test_argument_errors():
    from transvae.image_io import ImagePrep, pack_uint8, to_uint8_grid
    prep = ImagePrep(16)
    ok = np.zeros((20, 20, 3), np.uint8)
    with pytest.raises(ValueError, match="image 1 has 4 channels"):
        prep([ok, np.zeros((20, 20, 4), np.uint8)])
    with pytest.raises(ValueError, match="image 2 has 1 channels"):
        prep([ok, ok, np.zeros((20, 20), np.uint8)])
    with pytest.raises(ValueError, match="image 1: 16x257 -> 16x16 is a down-scale by more than 16"):
        ImagePrep(resize=(16, 16)).describe(torch.tensor([[0, 20, 20, 60, 3], [1200, 16, 257, 771, 3]]))
    with pytest.raises(ValueError, match="image 1: 400x20 -> 16x16 is a down-scale by more than 16"):
        ImagePrep(resize=(16, 16))([ok, np.zeros((400, 20, 3), np.uint8)])
    with pytest.raises(ValueError, match="image 0 is empty"):
        prep.describe(torch.tensor([[0, 0, 20, 60, 3]]))
    ImagePrep(resize=(16, 16)).describe(torch.tensor([[0, 256, 256, 768, 3]]))       # ratio 16 exactly is supported
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prep([torch.zeros(20, 20, 3, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prep(torch.zeros(2, 20, 20, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prep(pack_uint8([ok], pin=False))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        to_uint8_grid(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError):
        to_uint8_grid(torch.zeros(2, 1, 4, 4))
    with pytest.raises(ValueError):
        to_uint8_grid(torch.zeros(2, 3, 4, 4), transform="tanh")
    with pytest.raises(ValueError):
        ImagePrep(16, range="bytes")
    with pytest.raises(ValueError):
        ImagePrep(0)


def test_public_surface():
    import inspect
    import transvae
    assert {"ImagePrep", "UInt8Batch", "collate_uint8", "to_uint8_grid", "save_image", "random_samples", "interpolate_latents",
            "reconstruct"} <= set(transvae.__all__)
    p = inspect.signature(transvae.evaluate).parameters["prep"]
    assert p.default is None
