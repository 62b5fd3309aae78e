"""The image pipeline on the MI355X (`-m gpu`).

`ImagePrep` against the PIL-minted golden (tests/golden/image_prep_pil.npz): every output value EQUAL, no tolerance -- as one
ragged batch in one launch and one image at a time, with padded row strides and odd starts, in the signed range, from a dense
tensor.  `to_uint8_grid` against the restatement (tests/image_restatement.py): equal with transform="none"; with the sigmoid,
equal except at pixels whose fp64 255 s + 0.5 lies within 1e-3 of an integer, where one level is allowed, the share of such
pixels being asserted under 1 %.  transvae.generate and evaluate(prep=...) on the micro model.
"""
import json
import os

import numpy as np
import pytest
import torch

import image_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep_pil.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    cases = json.loads(bytes(g["cases"]).decode())
    groups = {}
    for c in cases:       # cases that share an output size form one ragged batch
        key = ("resize",) + tuple(c["resize"]) if "resize" in c else ("res", c["res"])
        groups.setdefault(key, []).append(c)
    assert sorted(k for k in groups if k[0] == "res") == [("res", 16), ("res", 32), ("res", 64), ("res", 72)]
    return g, groups


def make_prep(key, **kw):
    from transvae.image_io import ImagePrep
    return ImagePrep(key[1], **kw) if key[0] == "res" else ImagePrep(resize=key[1:], **kw)


def expected(g, cases, signed=False):
    return torch.stack([R.to_tensor(g["out_" + c["name"]], signed) for c in cases])


def test_ragged_batch_equals_pil_in_one_launch(golden):
    g, groups = golden
    for key, cases in groups.items():
        prep = make_prep(key)
        imgs = [torch.from_numpy(g["in_" + c["name"]]).to(DEV) for c in cases]
        out = prep(imgs)
        want = expected(g, cases)
        assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == tuple(want.shape)
        got = out.cpu()
        for i, c in enumerate(cases):
            assert torch.equal(got[i], want[i]), (c["name"], float((got[i] - want[i]).abs().max()) * 255)


def test_one_image_at_a_time_equals_pil(golden):
    g, groups = golden
    for key, cases in groups.items():
        prep = make_prep(key)
        for c in cases:
            out = prep([torch.from_numpy(g["in_" + c["name"]]).to(DEV)])
            assert torch.equal(out.cpu(), expected(g, [c])), c["name"]


def test_padded_rows_and_odd_starts_give_the_same_bits(golden):
    from transvae.image_io import pack_uint8
    g, groups = golden
    for key, cases in groups.items():
        prep = make_prep(key)
        arrays = [g["in_" + c["name"]] for c in cases]
        want = expected(g, cases)
        tight = pack_uint8(arrays)
        padded = pack_uint8(arrays, row_pad=5)
        shifted = pack_uint8(arrays, align=2, row_pad=1)
        shifted.data = torch.cat([torch.zeros(1, dtype=torch.uint8), shifted.data])     # every image now starts at an odd byte
        shifted.table[:, 0] += 1
        assert all(int(o) % 2 == 1 for o in shifted.table[:, 0])
        for name, batch in (("tight", tight), ("padded", padded), ("shifted", shifted)):
            assert torch.equal(prep(batch.to(DEV)).cpu(), want), (key, name)


def test_signed_range_and_dense_input(golden):
    g, groups = golden
    key = ("res", 16)
    cases = groups[key]
    imgs = [torch.from_numpy(g["in_" + c["name"]]).to(DEV) for c in cases]
    unit = make_prep(key)(imgs)
    signed = make_prep(key, range="signed")(imgs)
    assert torch.equal(signed, unit * 2 - 1) and torch.equal(signed.cpu(), expected(g, cases, signed=True))
    same = [c for c in cases if (c["h"], c["w"]) == (37, 53)]
    assert len(same) >= 2
    dense = torch.stack([torch.from_numpy(g["in_" + c["name"]]) for c in same]).to(DEV)
    assert torch.equal(make_prep(key)(dense), make_prep(key)([d for d in dense]))
    assert torch.equal(make_prep(key)(dense).cpu(), expected(g, same))
    wide = torch.zeros(len(same), 37, 60, 3, dtype=torch.uint8, device=DEV)        # a strided view is read in place
    wide[:, :, :53] = dense
    assert torch.equal(make_prep(key)(wide[:, :, :53]).cpu(), expected(g, same))


def test_unsupported_images_name_their_index():
    from transvae.image_io import ImagePrep
    ok = torch.zeros(20, 20, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="image 1"):
        ImagePrep(resize=(16, 16))([ok, torch.zeros(400, 20, 3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(ValueError, match="image 1 has 4 channels"):
        ImagePrep(16)([ok, torch.zeros(20, 20, 4, dtype=torch.uint8, device=DEV)])
    out = ImagePrep(16)([ok])
    assert tuple(out.shape) == (1, 3, 16, 16) and float(out.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
def grid_input(B, H=13, W=17, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g) * 0.6 + 0.5          # values below 0 and above 1
    flat = x.view(-1)
    n = flat.numel()
    ties = torch.arange(256, dtype=torch.float32) / 255            # exact k/255: x*255 + 0.5 is k + 0.5 up to rounding
    flat[:256] = ties
    flat[256:512] = (torch.arange(256, dtype=torch.float32) + 0.5) / 255   # the truncation boundaries themselves
    flat[n - 3:] = float("nan")
    flat[n - 5] = float("inf")
    flat[n - 6] = float("-inf")
    finite = x[torch.isfinite(x)]
    assert finite.min() < 0 and finite.max() > 1
    return x


@pytest.mark.parametrize("B", [1, 5, 8])
def test_grid_equals_restatement(B):
    from transvae.image_io import to_uint8_grid
    x = grid_input(B, seed=B)
    for nrow in (4, 8):
        for padding in (0, 2):
            want = R.grid_u8(x, nrow, padding, 0.0)
            for xd in (x.to(DEV), x.to(DEV).contiguous(memory_format=torch.channels_last)):
                got = to_uint8_grid(xd, nrow=nrow, padding=padding)
                assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
                assert np.array_equal(got.cpu().numpy(), want), (B, nrow, padding, xd.is_contiguous())
    want = R.grid_u8(x, 4, 2, 0.5)
    assert np.array_equal(to_uint8_grid(x.to(DEV), nrow=4, padding=2, pad_value=0.5).cpu().numpy(), want)


def test_grid_sigmoid_against_fp64():
    from transvae.image_io import to_uint8_grid
    x = torch.randn(8, 3, 32, 40, generator=torch.Generator().manual_seed(11))
    want, near, share = R.grid_u8_sigmoid_fp64(x, nrow=4, padding=2)
    assert share < 0.01, share              # the allowance below covers under 1 % of the input (about 0.2 % expected)
    got = to_uint8_grid(x.to(DEV), nrow=4, padding=2, transform="sigmoid").cpu().numpy()
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert (diff[~near] == 0).all(), int((diff[~near] != 0).sum())
    assert (diff[near] <= 1).all()


def test_save_image_writes_the_grid(tmp_path):
    from transvae.image_io import save_image, to_uint8_grid
    x = grid_input(5, seed=3).to(DEV)
    save_image(x, tmp_path / "a.png", nrow=4, padding=2)
    assert np.array_equal(R.decode_png((tmp_path / "a.png").read_bytes()), to_uint8_grid(x, nrow=4, padding=2).cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def micro():
    from oracle import filler
    from oracle import transvae_oracle as O
    from transvae import TransVAE
    cfg = dict(O.MICRO)
    m = TransVAE(config=cfg, variant="micro", compression_ratio=16, latent_dim=4)
    m.load_state_dict(filler.fill_state_dict(O.state_dict_schema(cfg, latent_dim=4)))
    return m.to(DEV)


def test_interpolate_latents_and_random_samples(micro):
    from transvae.generate import interpolate_latents, random_samples

    class Wrapped(torch.nn.Module):          # a DDP-style wrapper: .module is unwrapped
        def __init__(self, module):
            super().__init__()
            self.module = module

    frames, latents = interpolate_latents(Wrapped(micro), 5, spatial_size=4, seed=21, return_latents=True)
    assert not micro.training
    torch.manual_seed(21)                    # the reference's formula, frame by frame
    z1 = torch.randn(1, 4, 4, 4, device=DEV)
    z2 = torch.randn(1, 4, 4, 4, device=DEV)
    ref = torch.cat([(1 - a) * z1 + a * z2 for a in torch.linspace(0, 1, 5, device=DEV)], dim=0)
    assert torch.equal(latents, ref)
    with torch.no_grad():
        assert torch.equal(frames, torch.sigmoid(micro.decoder(latents)))
    assert tuple(frames.shape) == (5, 3, 64, 64)
    a = random_samples(micro, 3, spatial_size=4, seed=5)
    b = random_samples(micro, 3, spatial_size=4, seed=5)
    assert torch.equal(a, b) and tuple(a.shape) == (3, 3, 64, 64) and float(a.min()) >= 0 and float(a.max()) <= 1
    assert not torch.equal(a, random_samples(micro, 3, spatial_size=4, seed=6))


def test_reconstruct_concatenates_along_width(micro):
    from transvae.generate import reconstruct
    x = torch.rand(2, 3, 64, 64, device=DEV)
    comparison, original, recon = reconstruct(micro, x)
    assert tuple(comparison.shape) == (2, 3, 64, 128) and original is x
    assert torch.equal(comparison[..., :64], x) and torch.equal(comparison[..., 64:], recon)
    assert float(recon.min()) >= 0 and float(recon.max()) <= 1


def test_evaluate_with_prep_equals_the_float_loader(micro):
    from transvae import ImagePrep, collate_uint8, evaluate
    rng = np.random.default_rng(17)
    sizes = [(40, 56), (56, 40), (32, 32), (33, 70)]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    floats = torch.stack([R.to_tensor(R.prep_uint8(im, res=32)) for im in images])
    uint8_loader = [collate_uint8([(images[0], 0), (images[1], 1)]), ([images[2], images[3]], torch.tensor([2, 3]))]
    float_loader = [(floats[:2], torch.tensor([0, 1])), (floats[2:], torch.tensor([2, 3]))]
    torch.manual_seed(99)
    got = evaluate(micro, uint8_loader, ("psnr", "ssim"), device=DEV, per_image=True, prep=ImagePrep(32))
    torch.manual_seed(99)
    want = evaluate(micro, float_loader, ("psnr", "ssim"), device=DEV, per_image=True)
    for k in ("psnr", "ssim"):
        assert np.array_equal(got[k]["values"], want[k]["values"]), k
        assert got[k]["mean"] == want[k]["mean"] and got[k]["std"] == want[k]["std"] and got[k]["median"] == want[k]["median"]
