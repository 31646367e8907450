"""The renderer's natural-content options (CPU): the default rendering is unchanged byte for byte, the texture is
sampled bilinearly with wrap-around, the photometry follows its formula per camera, and the photometric variants of
tests/_natural.py produce the content the GPU tests rely on."""
import builtins
import os

import numpy as np
import pytest
import torch

import _natural

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "stereo_quad_160x96.npz"))


def test_default_rendering_reproduces_the_golden_frames(synth):
    """make_golden.py's call re-rendered: L0, R0, L1, R1 of the stored quad, byte for byte (the golden quad,
    bench.py and every parity test consume the default rendering)."""
    seq = synth.StereoSequence(width=160, height=96, n_frames=2, seed=42, scales=(0.5, 2.0, 8.0), supersample=2)
    (L0, R0), (L1, R1) = [tuple(x.numpy() for x in seq.render(t)) for t in range(2)]
    for k, v in zip(("L0", "R0", "L1", "R1"), (L0, R0, L1, R1)):
        assert v.tobytes() == G[k].tobytes(), k


def test_explicit_identity_options_render_the_default(synth):
    kw = dict(width=208, height=64, n_frames=2, seed=11)
    a = synth.StereoSequence(**kw)
    b = synth.StereoSequence(texture=None, gain=(1.0, 1.0), offset=(0.0, 0.0), gamma=(1.0, 1.0), **kw)
    for t in range(2):
        for x, y in zip(a.render(t), b.render(t)):
            assert x.numpy().tobytes() == y.numpy().tobytes()


def test_texture_sampling_is_bilinear_with_wrap_around(synth):
    rng = np.random.default_rng(0)
    tex = rng.uniform(0, 1, (7, 11)).astype(np.float32)
    seq = synth.StereoSequence(width=64, height=32, n_frames=1, texture=tex, texel=0.5)
    # plane 0 starts at texel (0, 0): texel centres return the texel values, also one period away
    iu = torch.tensor([0, 3, 10, 11 + 3, -11 + 2], dtype=torch.float32)
    iv = torch.tensor([0, 6, 2, 7 + 6, -7 + 1], dtype=torch.float32)
    got = seq._texture(iu * 0.5, iv * 0.5, 0).numpy()
    want = tex[np.asarray(iv, int) % 7, np.asarray(iu, int) % 11]
    assert np.allclose(got, want, atol=1e-6)
    # between texels: the bilinear blend, including across the wrap seam (u between texel 10 and texel 0)
    u = torch.tensor([10.25, 2.5], dtype=torch.float32)
    v = torch.tensor([6.75, 3.5], dtype=torch.float32)
    got = seq._texture(u * 0.5, v * 0.5, 0).numpy()

    def bil(uu, vv):
        u0, v0 = int(np.floor(uu)), int(np.floor(vv))
        a, b = uu - u0, vv - v0
        t = lambda i, j: float(tex[j % 7, i % 11])   # noqa: E731
        return (t(u0, v0) * (1 - a) + t(u0 + 1, v0) * a) * (1 - b) + (t(u0, v0 + 1) * (1 - a) + t(u0 + 1, v0 + 1) * a) * b
    assert np.allclose(got, [bil(10.25, 6.75), bil(2.5, 3.5)], atol=1e-6)
    # planes start at different offsets into the image
    assert not np.allclose(seq._texture(iu, iv, 0).numpy(), seq._texture(iu, iv, 1).numpy())
    with pytest.raises(AssertionError):
        synth.StereoSequence(width=64, height=32, n_frames=1, texture=tex * 2.0)


def test_photometry_per_camera(synth):
    kw = dict(width=160, height=48, n_frames=1, seed=3, texture=_natural.texture("pink"))
    L, R = (x.numpy().astype(np.float64) for x in synth.StereoSequence(**kw).render(0))
    gL, gR = (x.numpy().astype(np.float64) for x in
              synth.StereoSequence(gain=(1.5, 0.5), offset=(0.0, 10.0), **kw).render(0))
    assert np.abs(gL - np.clip(1.5 * L, 0, 255)).max() <= 1.0          # one rounding of the reference image, times 1.5
    assert np.abs(gR - np.clip(0.5 * R + 10.0, 0, 255)).max() <= 1.0
    cL, _ = (x.numpy().astype(np.float64) for x in synth.StereoSequence(gamma=(0.5, 1.0), **kw).render(0))
    assert np.abs(cL - 255.0 * np.sqrt(L / 255.0)).max() <= 8.5         # sqrt's slope near 0 magnifies the rounding


def test_pink_noise_texture():
    a = _natural.pink_noise()
    assert a.shape == (512, 512) and a.dtype == np.float32 and a.min() == 0.0 and a.max() == 1.0
    assert np.array_equal(a, _natural.pink_noise())                    # deterministic
    # the power spectrum falls as 1/f^2: fit the slope of the radially averaged spectrum
    p = np.abs(np.fft.fft2(a - a.mean())) ** 2
    f = np.hypot(*np.meshgrid(np.fft.fftfreq(512), np.fft.fftfreq(512)))
    bins = np.geomspace(4 / 512, 128 / 512, 12)
    idx = np.digitize(f, bins)
    mids = [f[idx == i].mean() for i in range(1, len(bins))]
    pw = [p[idx == i].mean() for i in range(1, len(bins))]
    slope = np.polyfit(np.log(mids), np.log(pw), 1)[0]
    assert -2.4 < slope < -1.6, slope


def test_photograph_loader_skips_naming_the_package(monkeypatch):
    real_import = builtins.__import__

    def no_pkg(name, *a, **k):
        if name.split(".")[0] in ("sklearn", "matplotlib"):
            raise ImportError(name)
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pkg)
    monkeypatch.setattr(_natural, "_CACHE", {})
    for name, pkg_name in (("china", "scikit-learn"), ("grace_hopper", "matplotlib")):
        with pytest.raises(pytest.skip.Exception, match=pkg_name):
            _natural.texture(name)
    assert _natural.texture("pink").shape == (512, 512)


@pytest.mark.parametrize("name", _natural.TEXTURES)
def test_photometric_variants_reach_their_bounds(synth, name):
    """The evidence of the variant table on CPU-rendered frames (the GPU tests assert it again on what they render)."""
    tex = _natural.texture(name)
    assert tex.dtype == np.float32 and tex.ndim == 2 and 0.0 <= tex.min() and tex.max() <= 1.0
    out = {}
    for var in _natural.VARIANTS:
        L, R = (x.numpy() for x in _natural.sequence(synth, name, var, n_frames=1).render(0))
        out[var] = (L, R)
    assert _natural.saturated_fraction(out["overexposed"][0]) >= 0.05
    assert max(out["night"][0].max(), out["night"][1].max()) <= 60
    assert out["lr_mismatch"][0].tobytes() == out["day"][0].tobytes()
    assert out["lr_mismatch"][1].astype(int).mean() > out["day"][1].astype(int).mean() + 8
