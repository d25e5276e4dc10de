"""The three shapes of host wrapper in rtp_bindings — a frame, an adaptive frame, the AOVs — against their device-pointer siblings into
buffers the test allocates itself, bit for bit, and a shard without rows through each of them.  16 x 8 pixels at 2 spp."""
import ctypes as C

import numpy as np
import pytest

import rtp_bindings as rb

pytestmark = pytest.mark.gpu
W, H = 16, 8
ADAPTIVE = dict(min_spp=2, batch_spp=2, max_spp=4)


@pytest.fixture(scope="module")
def scene():
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(half_extent=1), device=0)
    yield dev, rb.rtiow_camera(W, H, 2, 8)
    dev.close()


def _same(got, want):
    got, want = np.ascontiguousarray(got), want.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def test_frame_is_its_sibling(scene):
    import torch
    dev, cam = scene
    fb = torch.full((H, W, 3), float("nan"), device="cuda:0")
    dev.render_lit(cam, fb.data_ptr(), lens=dict(lens_radius=0.05), sample_first=3)
    _same(dev.render_lit_to_host(cam, lens=dict(lens_radius=0.05), sample_first=3)[0], fb)
    dev.render(cam, fb.data_ptr(), sample_first=5)
    _same(dev.render_to_host(cam, sample_first=5)[0], fb)


def test_adaptive_frame_with_a_prior_is_its_sibling(scene):
    import torch
    dev, cam = scene
    prior = np.empty((H, W, 2), np.float32)
    prior[..., 0], prior[..., 1] = 4.0, 0.01
    fb = torch.full((H, W, 3), float("nan"), device="cuda:0")
    spp = torch.full((H, W), -1, dtype=torch.int32, device="cuda:0")
    mom = torch.full((H, W, 2), float("nan"), device="cuda:0")
    d_prior = torch.from_numpy(prior).to("cuda:0")
    for rule in (None, 1):
        params = dict(ADAPTIVE) if rule is None else dict(ADAPTIVE, rule=rule)
        dev.render_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), prior=d_prior.data_ptr(), **params)
        got = dev.render_adaptive_to_host(cam, prior=prior, **params)
        for g, w in zip(got[:3], (fb, spp, mom)):
            _same(g, w)
        assert int(got[1].min()) >= 2 and int(got[1].max()) <= 4


def test_aovs_are_their_sibling(scene):
    import torch
    dev, cam = scene
    bufs = {key: torch.zeros((H, W, per) if per > 1 else (H, W), dtype=getattr(torch, np.dtype(dtype).name), device="cuda:0")
            for key, _, dtype, per in rb.AOV_CHANNELS if dtype != np.uint32}
    hits = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")          # (the uint32 counts, held as 32-bit words)
    dev.render_aov(cam, {**{k: b.data_ptr() for k, b in bufs.items()}, "hits": hits.data_ptr()})
    got, _ = dev.render_aov_to_host(cam)
    for key, b in bufs.items():
        _same(got[key], b)
    _same(got["hits"].view(np.int32), hits)
    assert int(got["hits"].max()) == 2


def test_a_shard_without_rows(scene):
    dev, cam = scene
    shard = rb.Shard(band_rows=8, num_parts=4, part=1)          # one band of 8 rows: part 0 has it all
    assert rb.amd_lib().rt_shard_rows(H, C.byref(shard)) == 0
    assert dev.render_to_host(cam, shard=shard)[0].shape == (0, W, 3)
    assert dev.render_to_host(cam, shard=shard, sample_first=2)[0].shape == (0, W, 3)
    assert dev.render_lit_to_host(cam, shard=shard)[0].shape == (0, W, 3)
    fb, spp, moments, _ = dev.render_adaptive_to_host(cam, shard=shard, **ADAPTIVE)
    assert fb.shape == (0, W, 3) and spp.shape == (0, W) and moments.shape == (0, W, 2)
