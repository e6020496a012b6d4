"""CPU: the numpy restatement of the denoising objective (tests/helpers/objective_refs.py) against the reference's own statements,
as tools/make_golden_objective.py ran them (tests/golden/objective_step.npz): noisy and target bit for bit, the losses by the
rule of tests/test_gpu_valid.py - the reference sums its fp32 terms in fp32, the helpers in float64, and the tool measured how
far the two lie apart (``f64_distance``); four times that is the allowance."""
import numpy as np
import pytest

from conftest import golden
from helpers import objective_refs as R


@pytest.fixture(scope="module")
def g():
    return golden("objective_step")


def _distance(g, key):
    keys = [str(k) for k in g["f64_distance_keys"]]
    return float(g["f64_distance"][keys.index(key)])


def test_fixture_geometry(g):
    assert tuple(g["frames"]) == R.FRAMES and tuple(g["t"]) == R.STEPS and int(g["seed"]) == R.SEED
    assert np.array_equal(g["noise_schedule"], np.linspace(1e-4, 0.05, 50))
    label, init, noise, predicted = R.inputs()
    assert label.shape == (R.B, 2, R.T, R.F) and label.dtype == np.float32
    mx = np.abs(init).reshape(R.B, 2, -1).argmax(axis=2)
    assert mx[1, 0] // R.F >= R.FRAMES[1]               # utterance 1, re plane: the maximum sits in a padding frame


@pytest.mark.parametrize("sigma", (False, True))
@pytest.mark.parametrize("mode", R.MODES)
def test_noising_bit_for_bit(g, mode, sigma):
    label, init, noise, _ = R.inputs()
    noisy, target, maxbuf = R.noising(label, init, R.STEPS, noise, mode, sigma)
    assert np.array_equal(noisy, g[R.case_key(mode, sigma) + "_noisy"])
    assert np.array_equal(target, g["target_sigma"] if sigma else noise)
    if sigma:
        assert np.array_equal(maxbuf, np.abs(init).reshape(R.B * 2, -1).max(axis=1)) and maxbuf[2] == np.float32(99.0) / np.float32(11)
        assert not np.array_equal(target, noise)


@pytest.mark.parametrize("mode", R.MODES)
def test_losses_within_four_f64_distances(g, mode):
    label, init, noise, predicted = R.inputs()
    frames = list(R.FRAMES)
    _, (com, _, com_mag) = R.spec_losses(predicted, noise, frames)
    _, target, maxbuf = R.noising(label, init, R.STEPS, noise, mode, True)
    _, sig = R.sigma_loss(predicted, target, init, maxbuf, frames)
    for key, got in ((R.case_key(mode, False) + "_com_mse", com), (R.case_key(mode, False) + "_com_mag_mse", com_mag),
                     (R.case_key(mode, True) + "_com_mse_sigma", sig)):
        want, allow = float(g[key]), 4 * _distance(g, key)
        print(key, "helper", got, "reference", want, "distance", abs(got - want) / want, "allowed", allow)
        assert abs(got - want) <= allow * want, key
