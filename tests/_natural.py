"""Helper of the natural-content tests (test infrastructure): textures and photometric variants for
synth.StereoSequence(texture=..., gain=..., offset=..., gamma=...).

  * two natural photographs that ship with installed packages, decoded at run time (nothing is committed: china.jpg
    carries CC-BY terms): sklearn's `datasets/images/china.jpg` and matplotlib's `grace_hopper.jpg` sample data, both
    converted to grey floats in [0, 1] by PIL;
  * a procedural 1/f ("pink noise") texture that needs no package, so part of the natural-content suite never skips.

A test that needs a photograph calls `texture(name)`, which skips with a reason naming the missing package."""
import os

import numpy as np
import pytest

NATURAL = ("china", "grace_hopper")
TEXTURES = NATURAL + ("pink",)

# photometric variants: keyword arguments of StereoSequence
VARIANTS = {
    "day": dict(),                                                  # identity
    "overexposed": dict(gain=1.8),                                  # >= 5 % of the pixels clip at 255
    # max <= 60 (255 * 0.23 < 59): contrast near FAST's threshold of 20.  At gain 0.15 FAST(20) finds at most a handful of
    # corners per frame on every texture here and each LK step would stop at stage 1 before tracking anything
    "night": dict(gain=0.23),
    "lr_mismatch": dict(gain=(1.0, 1.1), offset=(0.0, 8.0)),        # no brightness constancy between the cameras
}


def _grey(path):
    from PIL import Image
    with Image.open(path) as im:
        g = np.asarray(im.convert("L"), dtype=np.float32) / 255.0
    return np.ascontiguousarray(g)


def _china_path():
    try:
        import sklearn
    except ImportError:
        pytest.skip("scikit-learn is not installed: it ships china.jpg")
    return os.path.join(os.path.dirname(sklearn.__file__), "datasets", "images", "china.jpg")


def _grace_hopper_path():
    try:
        import matplotlib.cbook
    except ImportError:
        pytest.skip("matplotlib is not installed: it ships grace_hopper.jpg")
    return matplotlib.cbook.get_sample_data("grace_hopper.jpg", asfileobj=False)


def pink_noise(n=512, seed=1, beta=1.0):
    """A square texture whose amplitude spectrum falls as 1/f**beta (natural-image statistics), normalised
    to [0, 1] by its 0.5 % and 99.5 % quantiles (clipped beyond)."""
    rng = np.random.default_rng(seed)
    fy = np.fft.fftfreq(n)[:, None]
    fx = np.fft.rfftfreq(n)[None, :]
    f = np.sqrt(fx * fx + fy * fy)
    f[0, 0] = 1.0
    spec = (rng.normal(size=f.shape) + 1j * rng.normal(size=f.shape)) / f ** beta
    spec[0, 0] = 0.0
    img = np.fft.irfft2(spec, s=(n, n))
    lo, hi = np.quantile(img, [0.005, 0.995])
    return np.ascontiguousarray(np.clip((img - lo) / (hi - lo), 0.0, 1.0), dtype=np.float32)


_CACHE = {}


def texture(name):
    """Grey float32 texture in [0, 1]; skips (with the package's name) if a photograph's package is missing."""
    if name not in _CACHE:
        if name == "china":
            _CACHE[name] = _grey(_china_path())
        elif name == "grace_hopper":
            _CACHE[name] = _grey(_grace_hopper_path())
        elif name == "pink":
            _CACHE[name] = pink_noise()
        else:
            raise KeyError(name)
    return _CACHE[name]


def sequence(synth, name, variant, width=1241, height=376, n_frames=13, device="cpu", seed=20200710):
    """A corridor walled with `name` under photometric `variant`."""
    return synth.StereoSequence(width=width, height=height, n_frames=n_frames, seed=seed, device=device,
                                texture=texture(name), **VARIANTS[variant])


def saturated_fraction(img):
    return float(np.mean(np.asarray(img) == 255))
