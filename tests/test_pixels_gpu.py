"""The device pixel path (csrc/pixel_ops.hip through cosmos_predict2.pixels) against the float64 truth of
tests/pixel_truth.py, the host path (pipeline.resize_input, the torch quantisations) and, end to end, the host
pipeline on the tiny nets."""
import numpy as np
import pytest
import torch

import pixel_truth as PT
from cosmos_predict2 import _native as N
from cosmos_predict2 import pixels
from cosmos_predict2.action_conditioned import ActionConditionedInference
from cosmos_predict2.net_config import tiny_dit
from cosmos_predict2.pipeline import Video2WorldInference, resize_input
from cosmos_predict2.vae import Wan2pt1VAEInterface, init_vae_state_dict

pytestmark = pytest.mark.gpu


def _src(hw, n=2, seed=0):
    g = torch.Generator().manual_seed(1000 * hw[0] + hw[1] + seed)
    return torch.randint(0, 256, (n, 3) + tuple(hw), generator=g, dtype=torch.uint8)


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("layout", ["TCHW", "THWC"])
@pytest.mark.parametrize("hw,target", PT.CASES)
def test_resize_matches_truth_and_host(device, hw, target, layout):
    src = _src(hw)
    truth = PT.resize_crop_truth(src.numpy(), target)
    host = resize_input(src, target).numpy()
    if layout == "TCHW":
        got = pixels.resize_input_device(src.to(device), target).cpu().numpy()
    else:
        thwc = src.permute(0, 2, 3, 1).contiguous().to(device)
        out = pixels.resize_input_device(thwc, target, layout="THWC")
        assert out.shape == (2,) + tuple(target) + (3,)
        got = out.permute(0, 3, 1, 2).cpu().numpy()
    ok = PT.check_bytes(got, truth, f"device {layout} {hw} -> {target}")
    assert np.array_equal(got[ok], host[ok])  # both obey the rule, so outside the tie band they are equal


def test_resize_exact_two_to_one(device):
    """(64, 96) -> (32, 48): the weights are 1/8, 3/8, 3/8, 1/8 (3/7, 3/7, 1/7 at the border), the interior sums are
    exact in fp32, and the bytes equal the host's, ties included (round half to even, not half up)."""
    src = _src((64, 96))
    host = resize_input(src, (32, 48))
    truth = PT.resize_crop_truth(src.numpy(), (32, 48))
    assert (np.abs(truth - np.floor(truth) - 0.5) == 0).sum() > 50  # exact ties are present
    for layout in ("TCHW", "THWC"):
        s = src.to(device) if layout == "TCHW" else src.permute(0, 2, 3, 1).contiguous().to(device)
        got = pixels.resize_input_device(s, (32, 48), layout=layout).cpu()
        got = got if layout == "TCHW" else got.permute(0, 3, 1, 2)
        assert torch.equal(got, host)
        PT.check_bytes(got.numpy(), truth, f"device {layout} 2:1")
        interior = (slice(None), slice(None), slice(1, -1), slice(1, -1))  # 1/8, 3/8 weights: exact in float64 too
        assert np.array_equal(got.numpy()[interior], np.rint(truth[interior]).astype(np.uint8))


def _tables(hin, win, rh, rw, device):
    return pixels.aa_tables(hin, rh, device), pixels.aa_tables(win, rw, device)


def test_resize_window_independent(device):
    src = _src((54, 96)).to(device)
    rh, rw = 32, 57
    ty, tx = _tables(54, 96, rh, rw, device)
    outs = {}
    for win in ((0, 0, rh, rw), (3, 5, 17, 29), (1, 0, 31, 45)):
        top, left, th, tw = win
        full = torch.zeros((2, 3, rh, rw), dtype=torch.uint8, device=device)
        N.resize_crop_u8(src, full[:, :, top: top + th, left: left + tw], ty, tx, win)
        outs[win] = full.cpu()
    ref = outs[(0, 0, rh, rw)]
    PT.check_bytes(ref.numpy(), PT.resize_truth(src.cpu().numpy(), rh, rw), "full extent")
    for (top, left, th, tw), o in outs.items():
        assert torch.equal(o[:, :, top: top + th, left: left + tw], ref[:, :, top: top + th, left: left + tw])


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("clast", [False, True])
def test_resize_stays_inside_its_bounds(device, n, clast):
    """Destination: a ragged window (31 x 45, odd row pitch) inside a buffer of 0xA5, which must stay 0xA5 outside
    the window. Source: a zero image inside a buffer of 255 (x / row strides no multiple of 4); any read outside the
    image would leak into the all-zero result."""
    hin, win_, rh, rw = 50, 75, 32, 48
    win = (1, 2, 31, 45)
    ty, tx = _tables(hin, win_, rh, rw, device)
    if clast:
        big = torch.full((n, hin + 6, win_ + 7, 3), 255, dtype=torch.uint8, device=device)
        src = big[:, 3: 3 + hin, 2: 2 + win_].permute(0, 3, 1, 2)
        dbig = torch.full((n, 40, 61, 3), 0xA5, dtype=torch.uint8, device=device)
        dst = dbig[:, 5: 5 + 31, 7: 7 + 45].permute(0, 3, 1, 2)
    else:
        big = torch.full((n, 3, hin + 6, win_ + 7), 255, dtype=torch.uint8, device=device)
        src = big[:, :, 3: 3 + hin, 2: 2 + win_]
        dbig = torch.full((n, 3, 40, 61), 0xA5, dtype=torch.uint8, device=device)
        dst = dbig[:, :, 5: 5 + 31, 7: 7 + 45]
    src.zero_()
    N.resize_crop_u8(src, dst, ty, tx, win)
    assert (dst == 0).all()
    keep = torch.ones_like(dbig, dtype=torch.bool)
    (keep[:, 5: 36, 7: 52] if clast else keep[:, :, 5: 36, 7: 52]).fill_(False)
    assert (dbig[keep] == 0xA5).all()
    # a strided x (every 3rd byte of a wider row: not a multiple of 4) takes the byte-by-byte path
    wide = torch.full((n, 3, hin, 3 * win_), 255, dtype=torch.uint8, device=device)
    wide[..., ::3] = 0
    dbig.fill_(0xA5)
    N.resize_crop_u8(wide[..., ::3], dst, ty, tx, win)
    assert (dst == 0).all() and (dbig[keep] == 0xA5).all()


def test_resize_rejections(device):
    t48 = pixels.aa_tables(48, 48, device)
    with pytest.raises(ValueError, match="more than 4"):  # ratio > 4: before any table or launch
        N.resize_crop_u8(torch.zeros(1, 3, 200, 48, dtype=torch.uint8, device=device),
                         torch.zeros(1, 3, 48, 48, dtype=torch.uint8, device=device), t48, t48, (0, 0, 48, 48))
    with pytest.raises(ValueError, match="more than 4"):
        pixels.resize_input_device(torch.zeros(1, 3, 160, 240, dtype=torch.uint8, device=device), (32, 48))  # 5:1
    with pytest.raises(ValueError, match="at most 4"):  # C = 5
        N.resize_crop_u8(torch.zeros(1, 5, 48, 48, dtype=torch.uint8, device=device),
                         torch.zeros(1, 5, 48, 48, dtype=torch.uint8, device=device), t48, t48, (0, 0, 48, 48))
    with pytest.raises(ValueError, match="uint8"):
        N.resize_crop_u8(torch.zeros(1, 3, 48, 48, dtype=torch.float32, device=device),
                         torch.zeros(1, 3, 48, 48, dtype=torch.uint8, device=device), t48, t48, (0, 0, 48, 48))
    with pytest.raises(ValueError, match="uint8"):
        pixels.resize_input_device(torch.zeros(1, 3, 48, 48, dtype=torch.int16, device=device), (32, 48))
    lib = N.load_library()  # and the library itself refuses them (-22) on the host
    z = torch.zeros(1, 5, 200, 48, dtype=torch.uint8, device=device)
    st = N._i64x4(z.stride())
    args = lambda C, hin: (z.data_ptr(), st, 1, C, hin, 48, z.data_ptr(), st, *(t.data_ptr() for t in t48), 1,  # noqa: E731
                           *(t.data_ptr() for t in t48), 1, 48, 48, 0, 0, 48, 48, None)
    assert lib.cp25_resize_crop_u8(*args(3, 200)) == -22
    assert lib.cp25_resize_crop_u8(*args(5, 48)) == -22


def test_process_video_frames_device(device):
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (7, 54, 96, 3), generator=g, dtype=torch.uint8)
    from cosmos_predict2.pipeline import process_video_frames

    for n in (1, 2):
        host = process_video_frames(frames, (32, 48), 9, n)
        got = pixels.process_video_frames_device(frames, (32, 48), 9, n, device=device)
        assert got.shape == host.shape and got.is_cuda
        truth = PT.resize_crop_truth(frames.permute(0, 3, 1, 2).numpy(), (32, 48))  # [7, 3, 32, 48]
        need = 4 * (n - 1) + 1
        idx = list(range(7 - need, 7)) + [6] * (9 - need)
        ok = PT.check_bytes(got[0].permute(1, 0, 2, 3).cpu().numpy(), truth[idx], f"video n={n}")
        assert np.array_equal(got[0].permute(1, 0, 2, 3).cpu().numpy()[ok], host[0].permute(1, 0, 2, 3).numpy()[ok])


# ------------------------------------------------------------------------------------------------ conversions
def _all_bf16():
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return bits[~torch.isnan(bits)]


def test_clip_to_u8_every_bf16_value(device):
    v = _all_bf16()
    assert v.numel() == 65282
    clip = torch.zeros(2 * 64 * 171 * 3, dtype=torch.bfloat16)
    clip[: v.numel()] = v
    clip = clip.view(2, 64, 171, 3)
    f = clip.float()
    want = ((f / 2.0 + 0.5).clamp(0.0, 1.0) * 255.0).to(torch.uint8)                 # AR write-back
    assert torch.equal(want, (torch.clamp((f + 1) / 2, 0, 1) * 255).to(torch.uint8))  # action loop
    assert torch.equal(want, (((1.0 + f) / 2) * 255.0).clamp(0, 255).to(torch.uint8))  # save_video
    d = clip.to(device)
    assert torch.equal(pixels.clip_to_uint8(d, "THWC").cpu(), want)
    nc = pixels.clip_to_uint8(d, "NCTHW")
    assert nc.shape == (1, 3, 2, 64, 171) and nc.is_contiguous()
    assert torch.equal(nc.cpu(), want.permute(3, 0, 1, 2)[None])
    # strided source: channels 1..3 of a 5-channel clip, every second column
    wide = torch.full((2, 64, 342, 5), 7.0, dtype=torch.bfloat16, device=device)
    wide[:, :, ::2, 1:4] = d
    out = torch.full((2, 64, 171, 3), 0xA5, dtype=torch.uint8, device=device)
    N.clip_to_u8(wide[:, :, ::2, 1:4], out)
    assert torch.equal(out.cpu(), want)


def test_u8_to_clip_every_value(device):
    g = torch.Generator().manual_seed(3)
    video = torch.stack([torch.arange(256, dtype=torch.uint8)[torch.randperm(256, generator=g)] for _ in range(3)])
    video = video.view(1, 3, 2, 8, 16)
    want = (video.to(torch.bfloat16) / 127.5 - 1.0)[0].permute(1, 2, 3, 0)  # [T, H, W, 3], evaluated on the CPU
    out = torch.full((2, 8, 16, 16), float("nan"), dtype=torch.bfloat16, device=device)
    N.u8_to_clip(video[0].to(device), out)
    assert torch.equal(out[..., :3].cpu(), want)
    assert (out[..., 3:].cpu().view(torch.int16) == 0).all()  # exact (positive) zeros over the garbage
    assert torch.equal(pixels.video_to_clip(video.to(device)).cpu(), out.cpu())
    # the same on the device's own torch arithmetic (what _normalize_video runs)
    dev = (video.to(device).to(torch.bfloat16) / 127.5 - 1.0)[0].permute(1, 2, 3, 0)
    assert torch.equal(out[..., :3], dev)
    # a strided [:, :, :px] slice of a longer video
    longer = torch.randint(0, 256, (1, 3, 5, 8, 16), generator=g, dtype=torch.uint8)
    got = pixels.video_to_clip(longer.to(device)[:, :, :1])
    assert torch.equal(got[..., :3].cpu(), (longer[:, :, :1].to(torch.bfloat16) / 127.5 - 1.0)[0].permute(1, 2, 3, 0))
    with pytest.raises(ValueError, match="uint8"):
        N.u8_to_clip(torch.zeros(3, 1, 8, 16, device=device))


# ------------------------------------------------------------------------------------------------ VAE
def test_vae_u8_entry_points(device):
    sd = init_vae_state_dict(seed=0)
    tok = Wan2pt1VAEInterface(sd, device=device, temporal_window=4)
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (1, 3, 9, 64, 96), generator=g, dtype=torch.uint8).to(device)
    norm = u8.to(torch.bfloat16) / 127.5 - 1.0  # model._normalize_video
    assert torch.equal(tok.encode_u8(u8), tok.encode(norm))
    assert torch.equal(tok.encode_u8(u8[:, :, :5]), tok.encode(norm[:, :, :5]))  # strided slice
    z = torch.randn(1, 16, 3, 8, 12, generator=g).to(device)
    want = ((tok.decode(z).float() / 2.0 + 0.5).clamp(0.0, 1.0) * 255.0).to(torch.uint8)  # [1, 3, T, H, W]
    assert len(want.unique()) > 2  # a picture, not one saturated value
    got = tok.decode_u8(z, "NCTHW")
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(tok.decode_u8(z, "THWC"), want[0].permute(1, 2, 3, 0))
    with pytest.raises(ValueError, match="layout"):
        tok.decode_u8(z, "CTHW")


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def pipes(device):
    kw = dict(device=device, net_cfg=tiny_dit(num_blocks=1), state_t=2)
    return Video2WorldInference("2B/post-trained", **kw), Video2WorldInference("2B/post-trained", pixel_path="device", **kw)


def test_ar_loop_device_equals_host(device, pipes):
    host, dev = pipes
    g = torch.Generator().manual_seed(11)
    vid = torch.randint(0, 256, (1, 3, 1, 64, 96), generator=g, dtype=torch.uint8)
    kw = dict(num_output_frames=8, chunk_size=5, chunk_overlap=1, num_latent_conditional_frames=1, resolution="64,96",
              seed=3, num_steps=2, guidance=3)
    ref = host.generate_autoregressive_from_batch("a prompt", vid, **kw)
    got = dev.generate_autoregressive_from_batch("a prompt", vid.to(device), return_uint8=True, **kw)
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == ref.shape == (1, 3, 8, 64, 96)
    want = ((ref / 2.0 + 0.5).clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    assert torch.equal(got.cpu(), want.cpu())
    with pytest.raises(ValueError, match="return_uint8"):
        host.generate_vid2world("a prompt", vid, return_uint8=True)


def test_image_input_device_equals_host(device, pipes, tmp_path):
    from PIL import Image

    host, dev = pipes
    img = np.random.RandomState(0).randint(0, 256, size=(128, 192, 3), dtype=np.uint8)  # exact 2:1 to (64, 96)
    Image.fromarray(img).save(tmp_path / "in.png")
    kw = dict(num_latent_conditional_frames=1, resolution="64,96", seed=1, num_steps=2, guidance=3)
    ref = host.generate_vid2world("a prompt", str(tmp_path / "in.png"), **kw)
    got = dev.generate_vid2world("a prompt", str(tmp_path / "in.png"), return_uint8=True, **kw)
    want = ((ref / 2.0 + 0.5).clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    assert got.shape == want.shape == (1, 3, 5, 64, 96) and torch.equal(got.cpu(), want.cpu())


def test_action_loop_device_equals_host(device):
    cfg = tiny_dit(num_blocks=1, action_dim=7, action_per_latent_frame=4)
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, size=(64, 80, 3), dtype=np.uint8)
    acts = rng.randn(24, 7).astype(np.float32)
    outs = []
    for path in ("host", "device"):
        pipe = Video2WorldInference("2B/robot/action-cond", device=device, net_cfg=cfg, pixel_path=path)
        outs.append(ActionConditionedInference(pipe).generate(img, acts, chunk_size=12, num_steps=2, guidance=7))
        del pipe
    assert outs[0].dtype == outs[1].dtype == np.uint8 and outs[0].shape == (25, 64, 80, 3)
    assert np.array_equal(outs[0], outs[1])


def test_inference_api_writes_the_same_mp4(device, pipes, tmp_path):
    """Inference over a device pipe writes its .mp4 from decode_u8's bytes: the same file content as the host pipe."""
    from PIL import Image

    from cosmos_predict2.config import InferenceArguments, SetupArguments
    from cosmos_predict2.inference import Inference
    from cosmos_predict2.video_io import read_mp4

    img = np.random.RandomState(2).randint(0, 256, size=(128, 192, 3), dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "in.png")
    vids = []
    for name, pipe in zip(("host", "device"), pipes):
        inf = object.__new__(Inference)  # the tiny pipes of this module instead of the 2B net Inference builds
        inf.setup_args = SetupArguments(output_dir=tmp_path / name, keep_going=False, pixel_path=name)
        inf.rank0, inf.pipe = True, pipe
        sample = InferenceArguments(name="i2w", inference_type="image2world", input_path=tmp_path / "in.png",
                                    prompt="A robot arm stacks two cubes.", resolution="64,96", num_output_frames=5,
                                    num_steps=2, guidance=3)
        paths = inf.generate([sample], tmp_path / name)
        vids.append(read_mp4(paths[0]))
    assert vids[0].shape == (5, 64, 96, 3) and np.array_equal(vids[0], vids[1])
