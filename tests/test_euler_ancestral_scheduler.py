"""EulerAncestralDiscreteScheduler on the CPU: the class reproduces the reference's own sampling loops (tests/golden/euler_ancestral,
written by scripts/make_euler_ancestral_golden.py), ``ancestral_coefficients`` is ``step`` as a linear map (every configuration, in
float64), the generator advances one draw per step, and what is not implemented is refused."""
import numpy as np
import pytest
import torch

from paddlemix_amd.schedulers import EulerAncestralDiscreteScheduler
from tests import euler_ancestral_cases as EC

U64 = 2.0 ** -53
TOL = dict(rtol=2e-5, atol=2e-6)   # tests/test_schedulers.py: scheduler against restatement loops


@pytest.mark.parametrize("name", list(EC.CONFIGS))
def test_product_class_reproduces_the_reference_sampling_loop(name):
    kw, steps, first = EC.CONFIGS[name]
    gold = np.load(EC.golden_path(name))
    lat, ts, sig, s0, zs = EC.toy_loop(EulerAncestralDiscreteScheduler(**kw), steps, first)
    assert np.array_equal(zs.numpy(), gold["noise"])   # the loop was stepped with the planes the reference was handed
    worst = {k: float(np.abs(np.asarray(v, dtype=np.float64) - gold[k]).max())
             for k, v in (("timesteps", ts), ("sigmas", sig), ("init_noise_sigma", s0), ("latents", lat.numpy()))}
    print(f"{name:<20} largest differences {worst}")
    sch = EulerAncestralDiscreteScheduler(**kw)
    sch.set_timesteps(steps)
    assert sch.timesteps.dtype == np.float32 and sch.sigmas.dtype == np.float32 and sch.sigmas[-1] == 0.0
    np.testing.assert_allclose(np.asarray(ts, dtype=np.float32), gold["timesteps"], **TOL)
    np.testing.assert_allclose(np.asarray(sig, dtype=np.float32), gold["sigmas"], **TOL)
    np.testing.assert_allclose(np.float32(s0), gold["init_noise_sigma"], **TOL)
    np.testing.assert_allclose(lat.numpy(), gold["latents"], **TOL)


def test_linspace_timesteps_are_not_rounded_and_the_initial_state_is_the_training_schedule():
    sch = EulerAncestralDiscreteScheduler(**EC.SD)
    assert len(sch) == 1000 and sch.order == 1 and sch.step_index is None
    assert sch.timesteps.dtype == np.float32 and sch.timesteps[0] == 999 and sch.timesteps[-1] == 0 and len(sch.timesteps) == 1000
    assert len(sch.sigmas) == 1001 and sch.sigmas[-1] == 0.0 and sch.init_noise_sigma == float(sch.sigmas.max())
    sch.set_timesteps(7)
    assert np.array_equal(sch.timesteps, np.linspace(0, 999, 7, dtype=np.float32)[::-1]) and sch.timesteps[1] != round(sch.timesteps[1])
    lead = EulerAncestralDiscreteScheduler(timestep_spacing="leading", steps_offset=1, **EC.SD)
    lead.set_timesteps(10)
    assert lead.timesteps.tolist() == [901, 801, 701, 601, 501, 401, 301, 201, 101, 1]
    assert lead.init_noise_sigma == (float(lead.sigmas.max()) ** 2 + 1) ** 0.5
    trail = EulerAncestralDiscreteScheduler(timestep_spacing="trailing", **EC.SD)
    trail.set_timesteps(4)
    assert trail.timesteps.tolist() == [999, 749, 499, 249] and trail.init_noise_sigma == float(trail.sigmas.max())


def test_img2img_start_takes_the_second_candidate_and_add_noise_is_x_plus_sigma_noise():
    sch = EulerAncestralDiscreteScheduler(**EC.SD)
    sch.set_timesteps(10)
    sch.timesteps = np.concatenate([sch.timesteps[:4], sch.timesteps[3:]])   # a duplicated timestep, as an order-2 schedule has
    sch.sigmas = np.concatenate([sch.sigmas[:4], sch.sigmas[3:]])
    sch._init_step_index(sch.timesteps[3])
    assert sch.step_index == 4
    sch.set_timesteps(10)
    g = torch.Generator().manual_seed(1)
    x, n = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    got = sch.add_noise(x, n, torch.tensor([sch.timesteps[3]] * 2))
    assert torch.equal(got, x + n * float(sch.sigmas[3]))
    assert sch.model_input_scale(sch.timesteps[3]) == 1.0 / (float(sch.sigmas[3]) ** 2 + 1) ** 0.5 and sch.step_index == 3
    assert torch.equal(sch.scale_model_input(x, sch.timesteps[3]), x / (float(sch.sigmas[3]) ** 2 + 1) ** 0.5)


@pytest.mark.parametrize("name", list(EC.CONFIGS))
def test_ancestral_coefficients_equal_step_in_float64(name):
    """a full loop on float64 tensors through step(); at every row a x + b e + c z on the same tensors. Both sides use the same float32
    sigma, sigma_up and dt and round in float64 only: step() forms x0, (x - x0) / sigma, the product with dt and two sums, a handful of
    roundings at |x|, |sigma e| / sigma and |c z|; 64 u64 of those magnitudes holds them all."""
    kw, steps, first = EC.CONFIGS[name]
    sch, lin = EulerAncestralDiscreteScheduler(**kw), EulerAncestralDiscreteScheduler(**kw)
    sch.set_timesteps(steps)
    lin.set_timesteps(steps)
    fresh = (lin._step_index, lin.timesteps.tolist(), lin.sigmas.tolist(), lin.num_inference_steps)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    worst, rows = 0.0, []
    for i, t in enumerate(sch.timesteps[first:], start=first):
        e, z = (torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(2))
        a, b, c = lin.ancestral_coefficients(t)
        want = sch.step(e, t, x, noise=z).prev_sample
        assert want.dtype == torch.float64 and lin.step_index == sch.step_index == i + 1
        got = a * x + b * e + c * z
        s = float(sch.sigmas[i])
        bound = 64 * U64 * (3 * x.abs() + (abs(b) + abs(s) + 1) * e.abs() + (c * z).abs())
        ratio = ((got - want).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio < 1.0, (name, i, ratio)
        assert all(np.isfinite(v) for v in (a, b, c)) and b < 0.0 <= c
        if kw.get("prediction_type", "epsilon") == "epsilon":
            assert a == 1.0
        rows.append((a, b, c))
        x = want
    print(f"{name:<20} worst |a x + b e + c z - step| / bound {worst:.3f} over {len(rows)} rows")
    assert rows[-1][2] == 0.0 and all(r[2] > 0.0 for r in rows[:-1])   # c == 0.0 exactly on the last row, and only there
    # the walk leaves the scheduler as set_timesteps left it once the index is reset (what the pipeline's plan does)
    lin._step_index = None
    assert fresh == (lin._step_index, lin.timesteps.tolist(), lin.sigmas.tolist(), lin.num_inference_steps)


def _loop(seed=None, noises=None, steps=6):
    sch = EulerAncestralDiscreteScheduler(**EC.SD)
    sch.set_timesteps(steps)
    g = None if seed is None else torch.Generator().manual_seed(seed)
    x = torch.ones(2, 4, 8, 8)
    for i, t in enumerate(sch.timesteps):
        x = sch.step(0.1 * x, t, x, generator=g, return_dict=False, **({} if noises is None else {"noise": noises[i]}))[0]
    return x, g


def test_generator_behaviour():
    a, ga = _loop(seed=5)
    b, gb = _loop(seed=5)
    c, _ = _loop(seed=6)
    assert torch.equal(a, b) and not torch.equal(a, c)               # the same seed, the same loop
    # one draw per step, the last included: the generator stands where six draws of the model output's shape leave it
    ref = torch.Generator().manual_seed(5)
    planes = [torch.randn(2, 4, 8, 8, generator=ref) for _ in range(6)]
    assert torch.equal(torch.randn(3, generator=ga), torch.randn(3, generator=ref))
    # noise= overrides the draw: the planes above give the seeded loop, and the generator is not touched
    d, _ = _loop(noises=planes)
    assert torch.equal(d, a)
    g = torch.Generator().manual_seed(9)
    before = g.get_state()
    sch = EulerAncestralDiscreteScheduler(**EC.SD)
    sch.set_timesteps(3)
    out = sch.step(torch.ones(1, 4), sch.timesteps[0], torch.ones(1, 4), generator=g, noise=torch.zeros(1, 4))
    assert torch.equal(g.get_state(), before) and hasattr(out, "pred_original_sample") and sch.step_index == 1


def test_refusals():
    with pytest.raises(NotImplementedError):
        EulerAncestralDiscreteScheduler(trained_betas=[0.1, 0.2])
    sch = EulerAncestralDiscreteScheduler(prediction_type="sample")
    sch.set_timesteps(4)
    x = torch.ones(1, 4)
    with pytest.raises(NotImplementedError, match="sample"):
        sch.step(x, sch.timesteps[0], x)
    with pytest.raises(NotImplementedError):
        sch.ancestral_coefficients(sch.timesteps[0])
    bad = EulerAncestralDiscreteScheduler(prediction_type="velocity")
    bad.set_timesteps(4)
    with pytest.raises(ValueError, match="must be one of `epsilon`, or `v_prediction`"):
        bad.step(x, bad.timesteps[0], x)
    with pytest.raises(ValueError, match="is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'."):
        EulerAncestralDiscreteScheduler(timestep_spacing="middle").set_timesteps(4)
    fresh = EulerAncestralDiscreteScheduler()
    with pytest.raises(ValueError, match="set_timesteps"):
        fresh.step(x, fresh.timesteps[0], x)
    ok = EulerAncestralDiscreteScheduler()
    ok.set_timesteps(4)
    with pytest.raises(ValueError, match="integer indices"):
        ok.step(x, 3, x)
