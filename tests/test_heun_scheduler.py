"""HeunDiscreteScheduler on the CPU: the class reproduces the reference's own sampling loops (tests/golden/heun, written by
scripts/make_heun_golden.py), ``heun_coefficients`` is ``step`` as a two-stage linear map (every configuration, in float64),
``coefficient_walk`` puts the state back, and what is not implemented is refused."""
import numpy as np
import pytest
import torch

from paddlemix_amd.schedulers import HeunDiscreteScheduler
from tests import heun_cases as HC

U64 = 2.0 ** -53
TOL = dict(rtol=2e-5, atol=2e-6)   # tests/test_euler_ancestral_scheduler.py: the same toy loop against the reference's class


@pytest.mark.parametrize("name", list(HC.CONFIGS))
def test_product_class_reproduces_the_reference_sampling_loop(name):
    """timesteps, sigmas and init_noise_sigma: BIT FOR BIT on every case (the class builds its tables in the reference's float32
    tensor arithmetic; no case needs the 1-ulp allowance). End latents: rtol 2e-5 / atol 2e-6 per element."""
    kw, steps, first = HC.CONFIGS[name]
    gold = np.load(HC.golden_path(name))
    lat, ts, sig, s0 = HC.toy_loop(HeunDiscreteScheduler(**kw), steps, first)
    worst = {k: float(np.abs(np.asarray(v, dtype=np.float64) - gold[k]).max())
             for k, v in (("timesteps", ts), ("sigmas", sig), ("init_noise_sigma", s0), ("latents", lat.numpy()))}
    print(f"{name:<22} largest differences {worst}")
    sch = HeunDiscreteScheduler(**kw)
    sch.set_timesteps(steps)
    assert sch.timesteps.dtype == np.float32 and sch.sigmas.dtype == np.float32 and sch.sigmas[-1] == 0.0
    assert len(sch.timesteps) == 2 * steps - 1 and len(sch.sigmas) == 2 * steps
    assert np.array_equal(np.asarray(ts, dtype=np.float32), gold["timesteps"])
    assert np.array_equal(np.asarray(sig, dtype=np.float32), gold["sigmas"])
    assert np.float32(s0) == gold["init_noise_sigma"]
    assert lat.dtype == torch.float32
    np.testing.assert_allclose(lat.numpy(), gold["latents"], **TOL)


def test_schedule_layout_spacings_and_the_initial_state():
    sch = HeunDiscreteScheduler()
    c = sch.config
    assert (c.beta_start, c.beta_end, c.beta_schedule, c.prediction_type, c.use_karras_sigmas, c.clip_sample, c.clip_sample_range,
            c.timestep_spacing, c.steps_offset) == (0.00085, 0.012, "linear", "epsilon", False, False, 1.0, "linspace", 0)
    assert len(sch) == 1000 and sch.order == 2 and sch.step_index is None and sch.state_in_first_order
    assert len(sch.timesteps) == 1999 and len(sch.sigmas) == 2000 and sch.timesteps[0] == 999 and sch.timesteps[-1] == 0
    sch = HeunDiscreteScheduler(**HC.SD)
    sch.set_timesteps(4)
    t = np.linspace(0, 999, 4, dtype=np.float32)[::-1]
    assert sch.timesteps.tolist() == [t[0], t[1], t[1], t[2], t[2], t[3], t[3]]
    s = sch.sigmas
    assert s[1] == s[2] and s[3] == s[4] and s[5] == s[6] and s[0] > s[1] > s[3] > s[5] > s[7] == 0.0
    assert sch.init_noise_sigma == float(s.max())
    lead = HeunDiscreteScheduler(timestep_spacing="leading", steps_offset=1, **HC.SD)
    lead.set_timesteps(5)
    assert lead.timesteps.tolist() == [801, 601, 601, 401, 401, 201, 201, 1, 1]
    m = np.float32(lead.sigmas.max())
    assert lead.init_noise_sigma == float(np.sqrt(m * m + np.float32(1)))
    trail = HeunDiscreteScheduler(timestep_spacing="trailing", **HC.SD)
    trail.set_timesteps(4)
    assert trail.timesteps.tolist() == [999, 749, 749, 499, 499, 249, 249]
    kar = HeunDiscreteScheduler(use_karras_sigmas=True, **HC.SD)
    kar.set_timesteps(6)
    assert len(kar.timesteps) == 11 and any(v != round(v) for v in kar.timesteps.tolist())   # from _sigma_to_t, not rounded
    rho = np.diff(kar.sigmas[[0, 1, 3, 5, 7, 9]].astype(np.float64) ** (1 / 7.0))
    assert np.allclose(rho, rho[0], rtol=1e-5)                                               # equal steps in sigma^(1/7)


def test_first_index_scale_model_input_and_add_noise_before_and_after_steps():
    sch = HeunDiscreteScheduler(**HC.SD)
    sch.set_timesteps(5)
    g = torch.Generator().manual_seed(1)
    x, n = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    t2 = sch.timesteps[3]                       # indices 3 and 4
    assert sch.index_for_timestep(t2) == 4 and sch.index_for_timestep(sch.timesteps[0]) == 0   # the second of two, the only one
    assert torch.equal(sch.add_noise(x, n, torch.tensor([t2, t2])), x + n * float(sch.sigmas[4]))
    assert sch.model_input_scale(t2) == 1.0 / (float(sch.sigmas[4]) ** 2 + 1) ** 0.5 and sch.step_index == 4   # an img2img start
    s4 = torch.tensor(float(sch.sigmas[4]))
    assert torch.equal(sch.scale_model_input(x, t2), x / ((s4 ** 2 + 1) ** 0.5))
    # after steps the counter of step() calls picks the index: one step at t1 taken -> its second index; none at t2 yet -> its first
    sch.set_timesteps(5)
    t0, t1 = sch.timesteps[0], sch.timesteps[1]
    y = sch.step(0.1 * x, t0, x).prev_sample
    y = sch.step(0.1 * y, t1, y).prev_sample
    assert sch.step_index == 2 and sch._index_counter == {float(t0): 1, float(t1): 1}
    assert sch.index_for_timestep(t1) == 2 and sch.index_for_timestep(t2) == 3
    assert torch.equal(sch.add_noise(x, n, torch.tensor([t1, t2])),
                       x + n * torch.tensor([float(sch.sigmas[2]), float(sch.sigmas[3])]).reshape(2, 1, 1, 1))
    sch.set_timesteps(5)
    assert sch._index_counter == {} and sch.step_index is None


def test_state_returns_to_first_order_after_every_pair_and_after_set_timesteps():
    sch = HeunDiscreteScheduler(**HC.SD)
    sch.set_timesteps(4)
    x = torch.ones(1, 4)
    for i, t in enumerate(sch.timesteps):
        assert sch.state_in_first_order == (i % 2 == 0)
        first = sch.state_in_first_order
        x = sch.step(0.1 * x, t, x, return_dict=False)[0]
        assert sch.step_index == i + 1
        if first:
            assert sch.dt is not None and sch.prev_derivative is not None and sch.sample is not None
        else:
            assert sch.dt is None and sch.prev_derivative is None and sch.sample is None
    assert not sch.state_in_first_order     # the last evaluation is a first-order step to sigma = 0: it parks, as the reference does
    sch.set_timesteps(4)
    assert sch.state_in_first_order and sch.prev_derivative is None and sch.sample is None and sch.step_index is None


def _reference_formulas(sch, e, x, i, state):
    """scheduling_heun_discrete.py step (:387-447) restated directly in float64 on the float32 sigmas -> prev; state: [d, dt, sample]"""
    c, sig = sch.config, sch.sigmas.astype(np.float64)
    first = state[1] is None
    sigma, sigma_next = (sig[i], sig[i + 1]) if first else (sig[i - 1], sig[i])
    s_in = sigma if first else sigma_next
    if c.prediction_type == "epsilon":
        x0 = x - s_in * e
    elif c.prediction_type == "v_prediction":
        x0 = e * (-s_in / (s_in ** 2 + 1) ** 0.5) + (x / (s_in ** 2 + 1))
    else:
        x0 = e
    if c.clip_sample:
        x0 = x0.clip(-c.clip_sample_range, c.clip_sample_range)
    if first:
        d = (x - x0) / sigma
        state[:] = [d, sigma_next - sigma, x]
        return x + d * (sigma_next - sigma)
    d = (state[0] + (x - x0) / sigma_next) / 2
    prev = state[2] + d * state[1]
    state[:] = [None, None, None]
    return prev


@pytest.mark.parametrize("kw", [dict(prediction_type="sample"), dict(clip_sample=True), dict(clip_sample=True, clip_sample_range=0.5),
                                dict(prediction_type="v_prediction", clip_sample=True), dict()])
def test_step_in_float64_stays_float64_and_follows_the_reference_formulas(kw):
    sch = HeunDiscreteScheduler(**HC.SD, **kw)
    sch.set_timesteps(6)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    want, state, worst = x.clone(), [None, None, None], 0.0
    for i, t in enumerate(sch.timesteps):
        e = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
        xin = sch.scale_model_input(x, t)
        assert xin.dtype == torch.float64
        x = sch.step(e, t, x).prev_sample
        want = _reference_formulas(sch, e, want, i, state)
        assert x.dtype == torch.float64 and sch.sigmas.dtype == np.float32
        worst = max(worst, float((x - want).abs().max() / want.abs().max()))
    print(f"{kw}: largest |step - restatement| / |latent| over the loop {worst:.2e}")
    assert worst < 1e-12       # both sides are float64 on the same float32 sigmas: only the order of a few operations can differ


@pytest.mark.parametrize("name", list(HC.CONFIGS) + ["sample_prediction"])
def test_heun_coefficients_equal_step_in_float64(name):
    """a full loop on float64 tensors through step(); at every row the two-stage linear map on the same tensors, with the parked
    sample and derivative carried as the kernel carries them. Both sides round in float64 only: step() forms x0, (x - x0) / sigma,
    the average and two products, a handful of roundings at |x|, |sigma e| / sigma and |h| |d|; 64 u64 of those magnitudes holds them
    all (for sample prediction 1 / sigma multiplies them)."""
    kw, steps, first = HC.CONFIGS[name] if name in HC.CONFIGS else (dict(HC.SD, prediction_type="sample"), 8, 0)
    sch, lin = HeunDiscreteScheduler(**kw), HeunDiscreteScheduler(**kw)
    sch.set_timesteps(steps)
    lin.set_timesteps(steps)
    fresh = (lin._step_index, lin.dt, lin.timesteps.tolist(), lin.sigmas.tolist(), lin.num_inference_steps)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    S = D = None
    worst, rows = 0.0, []
    with lin.coefficient_walk():
        for i, t in enumerate(sch.timesteps[first:], start=first):
            e = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
            scale = lin.model_input_scale(t)
            assert scale == 1.0 / (float(sch.sigmas[i]) ** 2 + 1) ** 0.5
            p, q, h, gg, second = lin.heun_coefficients(t)
            want = sch.step(e, t, x).prev_sample
            assert want.dtype == torch.float64 and lin.step_index == sch.step_index == i + 1
            assert lin.state_in_first_order == sch.state_in_first_order
            d = p * x + q * e
            if second == 0.0:
                got, S, D = x + h * d, x, d
                mags = x.abs() + abs(h) * ((abs(p) + 1) * x.abs() + (abs(q) + 1) * e.abs())
            else:
                got = S + h * (gg * D + d)
                mags = S.abs() + abs(h) * (D.abs() + (abs(p) + 1) * x.abs() + (abs(q) + 1) * e.abs())
            ratio = ((got - want).abs() / (64 * U64 * mags)).max().item()
            worst = max(worst, ratio)
            assert ratio < 1.0, (name, i, ratio)
            assert (second, gg) == ((0.0, 0.0) if i % 2 == 0 else (1.0, 1.0)) and h < 0.0
            if kw.get("prediction_type", "epsilon") == "epsilon":
                assert (p, q) == (0.0, 1.0)
            rows.append((p, q, h, gg, second))
            x = want
    print(f"{name:<22} worst |rows - step| / bound {worst:.3f} over {len(rows)} rows")
    assert rows[-1][4] == 0.0 and len(rows) == 2 * steps - 1 - first                      # the last row: stage 1, to sigma = 0
    assert all(b[2] == a[2] / 2 for a, b in zip(rows[0::2], rows[1::2]))                   # stage 2 takes half the parked dt
    # coefficient_walk put back what the walk advanced: the scheduler is as set_timesteps left it
    assert fresh == (lin._step_index, lin.dt, lin.timesteps.tolist(), lin.sigmas.tolist(), lin.num_inference_steps)
    assert lin.state_in_first_order


def test_coefficient_walk_restores_a_mid_loop_state():
    sch = HeunDiscreteScheduler(**HC.SD)
    sch.set_timesteps(4)
    x = torch.ones(1, 4)
    x = sch.step(0.1 * x, sch.timesteps[0], x).prev_sample     # parked: second order next
    before = (sch.step_index, sch.dt, sch.prev_derivative, sch.sample)
    with sch.coefficient_walk():
        row = sch.heun_coefficients(sch.timesteps[1])
        assert row[4] == 1.0 and row[2] == float(before[1]) / 2 and sch.state_in_first_order and sch.step_index == 2
    assert (sch.step_index, sch.prev_derivative, sch.sample) == (before[0], before[2], before[3]) and sch.dt is before[1]


def test_refusals():
    with pytest.raises(NotImplementedError):
        HeunDiscreteScheduler(trained_betas=[0.1, 0.2])
    with pytest.raises(NotImplementedError, match="squaredcos_cap_v2"):
        HeunDiscreteScheduler(beta_schedule="squaredcos_cap_v2")
    x = torch.ones(1, 4)
    bad = HeunDiscreteScheduler(prediction_type="velocity")
    bad.set_timesteps(4)
    with pytest.raises(ValueError, match="must be one of `epsilon`, or `v_prediction`"):
        bad.step(x, bad.timesteps[0], x)
    with pytest.raises(ValueError, match="must be one of `epsilon`, or `v_prediction`"):
        bad.heun_coefficients(bad.timesteps[0])
    with pytest.raises(ValueError, match="is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'."):
        HeunDiscreteScheduler(timestep_spacing="middle")
    clip = HeunDiscreteScheduler(clip_sample=True)
    clip.set_timesteps(4)
    with pytest.raises(NotImplementedError, match="clip_sample"):
        clip.heun_coefficients(clip.timesteps[0])
    assert clip.step_index is None or clip.state_in_first_order
    assert torch.isfinite(clip.step(x, clip.timesteps[0], x).prev_sample).all()     # the generic step clips
