"""KDPM2DiscreteScheduler and KDPM2AncestralDiscreteScheduler on the CPU: the classes reproduce the reference's own sampling loops
(tests/golden/dpm2, written by scripts/make_dpm2_golden.py), ``dpm2_coefficients`` is ``step`` as a two-stage linear map,
``coefficient_walk`` puts the state back, the ancestral ``step`` draws once per evaluation, and what is not implemented is refused."""
import numpy as np
import pytest
import torch

from paddlemix_amd.schedulers import KDPM2AncestralDiscreteScheduler, KDPM2DiscreteScheduler
from tests import dpm2_cases as DC

TOL = dict(rtol=2e-5, atol=2e-6)   # the project's tolerance for reference loops (tests/test_heun_scheduler.py)
CLS = {False: KDPM2DiscreteScheduler, True: KDPM2AncestralDiscreteScheduler}
BOTH = pytest.mark.parametrize("anc", [False, True], ids=["dpm2", "dpm2a"])


@pytest.mark.parametrize("name", list(DC.CONFIGS))
def test_product_class_reproduces_the_reference_sampling_loop(name):
    """timesteps, every schedule table and init_noise_sigma: BIT FOR BIT on every case (NaN where the reference has NaN: entries no
    evaluation reads). End latents: rtol 2e-5 / atol 2e-6 per element (bit equality is reached too, see the README; not asserted)."""
    anc, kw, steps, first = DC.CONFIGS[name]
    gold = np.load(DC.golden_path(name))
    lat, ts, tabs, s0, zs = DC.toy_loop(CLS[anc](**kw), steps, first, ancestral=anc)
    assert set(tabs) == set(DC.TABLES if anc else DC.TABLES[:2]) <= set(gold.files)
    print(f"{name:<22} largest latent difference {float(np.abs(lat.numpy() - gold['latents']).max()):.3g}")
    sch = CLS[anc](**kw)
    sch.set_timesteps(steps)
    assert sch.timesteps.dtype == np.float32 and sch.sigmas.dtype == np.float32 and sch.sigmas[-1] == 0.0
    assert len(sch.timesteps) == 2 * steps - 1 and len(sch.sigmas) == 2 * steps + 2
    assert np.array_equal(np.asarray(ts, dtype=np.float32), gold["timesteps"])
    for k, v in tabs.items():
        assert np.array_equal(np.asarray(v, dtype=np.float32), gold[k], equal_nan=True), k
    assert np.float32(s0) == gold["init_noise_sigma"]
    if anc:
        assert np.array_equal(zs.numpy(), gold["noise"]) and len(zs) == 2 * steps - 1 - first   # one plane per evaluation
    assert lat.dtype == torch.float32
    np.testing.assert_allclose(lat.numpy(), gold["latents"], **TOL)


@pytest.mark.parametrize("name", list(DC.CONFIGS))
def test_live_comparison_with_the_reference(name):
    """when the reference checkout is present: its class, run now, against the recorded file and the product class"""
    from oracle import reference_runner as rr
    if not rr.available():
        pytest.skip("the reference checkout is not present")
    from oracle import paddle_shim
    anc, kw, steps, first = DC.CONFIGS[name]
    had = {k: paddle_shim.Tensor.__dict__.get(k) for k in ("roll", "lerp")}
    paddle_shim.Tensor.roll = lambda self, shifts, axis=None: paddle_shim.Tensor(torch.roll(self.t, shifts, axis))
    paddle_shim.Tensor.lerp = lambda self, y, weight: paddle_shim.Tensor(torch.lerp(self.t, rr.from_shim(y), weight))
    mod = rr.ref_module("scheduling_k_dpm_2_ancestral_discrete" if anc else "scheduling_k_dpm_2_discrete", "schedulers")
    ref = getattr(mod, CLS[anc].__name__)
    randn = getattr(mod, "randn_tensor", None)

    def step(sch, eps, t, x, z):
        if anc:
            mod.randn_tensor = lambda shape, generator=None, dtype=None, **_: z
        return sch.step(eps, t, x, return_dict=False)[0]
    try:
        lat = DC.toy_loop(ref(**kw), steps, first, wrap=rr.to_shim, unwrap=rr.from_shim, step=step)[0]
    finally:
        for k, v in had.items():
            if v is None:
                delattr(paddle_shim.Tensor, k)
        if randn is not None:
            mod.randn_tensor = randn
    assert np.array_equal(lat.numpy(), np.load(DC.golden_path(name))["latents"])
    own = DC.toy_loop(CLS[anc](**kw), steps, first, ancestral=anc)[0]
    np.testing.assert_allclose(own.numpy(), lat.numpy(), **TOL)


@BOTH
def test_schedule_layout_spacings_and_the_initial_state(anc):
    sch = CLS[anc]()
    c = sch.config
    assert (c.num_train_timesteps, c.beta_start, c.beta_end, c.beta_schedule, c.trained_betas, c.use_karras_sigmas, c.prediction_type,
            c.timestep_spacing, c.steps_offset) == (1000, 0.00085, 0.012, "linear", None, False, "epsilon", "linspace", 0)
    assert len(sch) == 1000 and sch.order == 2 and sch.step_index is None and sch.state_in_first_order
    assert len(sch.timesteps) == 1999 and len(sch.sigmas) == 2002 and sch.timesteps[0] == 999 and sch.timesteps[-1] == 0
    sch = CLS[anc](**DC.SD)
    sch.set_timesteps(4)
    t = np.linspace(0, 999, 4, dtype=np.float32)[::-1]
    assert sch.timesteps[0::2].tolist() == t.tolist() and len(sch.timesteps) == 7
    # the midpoint timesteps lie below their step's; above the next step's for DPM2 (DPM2 a's midpoint, between sigma and sigma_down,
    # may lie below sigma_next)
    assert all(t[k] > sch.timesteps[2 * k + 1] and (anc or sch.timesteps[2 * k + 1] > t[k + 1]) for k in range(3))
    assert any(v != round(v) for v in sch.timesteps[1::2].tolist())                # from _sigma_to_t, not rounded
    s, si = sch.sigmas, sch.sigmas_interpol
    assert s[1] == s[2] and s[3] == s[4] and s[5] == s[6] and s[0] > s[1] > s[3] > s[5] > s[7] == s[8] == s[9] == 0.0
    assert sch.init_noise_sigma == float(s.max())
    if anc:   # the midpoint of step k: between sigma_k and sigma_down_k (log-linear), at index 2k; the last step goes to 0
        sd, su = sch.sigmas_down, sch.sigmas_up
        for k, i in enumerate((0, 1, 3)):
            assert s[i] > si[i] > sd[i] > 0.0 and su[i] > 0.0
            assert abs(si[i] - np.sqrt(np.float64(s[i]) * sd[i])) < 1e-6 * si[i]
            assert abs(np.float64(sd[i]) ** 2 + np.float64(su[i]) ** 2 - np.float64(s[2 * k + 1]) ** 2) < 1e-5 * s[2 * k + 1] ** 2
        assert si[5] == 0.0 and sd[5] == 0.0 and su[5] == 0.0
    else:     # the midpoint of step k: the geometric mean of sigma_k and sigma_{k+1}, at index 2k + 1; the last step goes to 0
        for i in (1, 3, 5):
            assert s[i - 1] > si[i] > s[i] and abs(si[i] - np.sqrt(np.float64(s[i - 1]) * s[i])) < 1e-6 * si[i]
        assert si[7] == 0.0
    lead = CLS[anc](timestep_spacing="leading", steps_offset=1, **DC.SD)
    lead.set_timesteps(5)
    assert lead.timesteps[0::2].tolist() == [801, 601, 401, 201, 1]
    m = np.float32(lead.sigmas.max())
    assert lead.init_noise_sigma == float(np.sqrt(m * m + np.float32(1)))
    trail = CLS[anc](timestep_spacing="trailing", **DC.SD)
    trail.set_timesteps(4)
    assert trail.timesteps[0::2].tolist() == [999, 749, 499, 249]
    kar = CLS[anc](use_karras_sigmas=True, **DC.SD)
    kar.set_timesteps(6)
    assert len(kar.timesteps) == 11 and all(v == round(v) for v in kar.timesteps[0::2].tolist())   # the steps' own ARE rounded here
    rho = np.diff(kar.sigmas[[0, 1, 3, 5, 7, 9]].astype(np.float64) ** (1 / 7.0))
    assert np.allclose(rho, rho[0], rtol=1e-5)                                                    # equal steps in sigma^(1/7)


@BOTH
def test_scale_model_input_uses_the_midpoint_sigma_on_a_second_stage_index(anc):
    sch = CLS[anc](**DC.SD)
    sch.set_timesteps(5)
    x = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    for i, t in enumerate(sch.timesteps[:4]):
        stage2 = i % 2 == 1
        sigma = float((sch.sigmas_interpol[i - 1 if anc else i]) if stage2 else sch.sigmas[i])
        assert sch.state_in_first_order == (not stage2)
        with sch.coefficient_walk():
            assert sch.model_input_scale(t) == 1.0 / (sigma ** 2 + 1) ** 0.5
        xin = sch.scale_model_input(x, t)
        assert torch.equal(xin, x / ((torch.tensor(sigma) ** 2 + 1) ** 0.5)) and sch.step_index == i
        x = sch.step(0.1 * xin, t, x).prev_sample
        assert sch.step_index == i + 1
    # an img2img start at an even index: add_noise takes sigmas[index], the first evaluation is a stage 1
    sch.set_timesteps(5)
    t4 = sch.timesteps[4]
    assert sch.index_for_timestep(t4) == 4 and sch.state_in_first_order
    n = torch.ones_like(x)
    assert torch.equal(sch.add_noise(x, n, torch.tensor([t4, t4])), x + n * float(sch.sigmas[4]))
    assert sch.model_input_scale(t4) == 1.0 / (float(sch.sigmas[4]) ** 2 + 1) ** 0.5 and sch.step_index == 4


@BOTH
def test_state_returns_to_first_order_after_every_pair_and_after_set_timesteps(anc):
    sch = CLS[anc](**DC.SD)
    sch.set_timesteps(4)
    x = torch.ones(1, 4)
    for i, t in enumerate(sch.timesteps):
        assert sch.state_in_first_order == (i % 2 == 0)
        x = sch.step(0.1 * x, t, x, return_dict=False)[0]
        assert sch.step_index == i + 1 and (sch.sample is None) == (i % 2 == 1)
    assert not sch.state_in_first_order     # the last evaluation is a first-order step to sigma = 0: it parks, as the reference does
    sch.set_timesteps(4)
    assert sch.state_in_first_order and sch.step_index is None and sch._index_counter == {}


def _rows_loop(rows, x, es, zs):
    """the loop rebuilt from the rows alone, float64: stage 1 parks x, stage 2 starts from it"""
    S = None
    for (p, q, h, c, second), e, z in zip(rows, es, zs):
        d = p * x + q * e
        if second == 0.0:
            S, x = x, x + h * d
        else:
            x = S + h * d + (c * z if c != 0.0 else 0.0)
    return x


@pytest.mark.parametrize("name", list(DC.CONFIGS) + ["dpm2_8_steps", "dpm2a_8_steps", "dpm2_8_steps_v", "dpm2a_8_steps_v"])
def test_loop_rebuilt_from_the_rows_equals_step_to_fp32_rounding(name):
    """``step`` on float32 tensors against the rows applied in float64 to the same model outputs and noise: the rows are composed in
    float64 from the float32 schedule values step uses, so only step's own float32 roundings separate the two -- about 10 per
    evaluation (x0, the derivative, dt, the products and sums), each at most u = 2^-24 of the largest magnitude of the loop (the
    start, ~ 15 sigma_max). 16 u per evaluation RUN bounds them with room; the walk leaves the scheduler as it found it."""
    if name in DC.CONFIGS:
        anc, kw, steps, first = DC.CONFIGS[name]
    else:
        anc, kw, steps, first = name.startswith("dpm2a"), dict(DC.SD, **(dict(prediction_type="v_prediction") if name.endswith("_v") else {})), 8, 0
    sch, lin = CLS[anc](**kw), CLS[anc](**kw)
    sch.set_timesteps(steps)
    lin.set_timesteps(steps)
    fresh = (lin._step_index, lin.sample, lin.timesteps.tolist(), lin.sigmas.tolist(), lin.num_inference_steps)
    with lin.coefficient_walk():
        scales_rows = [(lin.model_input_scale(t), lin.dpm2_coefficients(t)) for t in lin.timesteps]
        assert lin.step_index == 2 * steps - 1 and not lin.state_in_first_order
    assert fresh == (lin._step_index, lin.sample, lin.timesteps.tolist(), lin.sigmas.tolist(), lin.num_inference_steps)
    assert lin.state_in_first_order and lin.step_index is None
    rows = [r for _, r in scales_rows]
    assert [r[4] for r in rows] == [float(i % 2) for i in range(2 * steps - 1)] and all(r[2] < 0.0 for r in rows)
    assert all((r[3] > 0.0) == (anc and r[4] == 1.0) for r in rows) and all(r[3] == 0.0 for r in rows if not (anc and r[4] == 1.0))
    if kw.get("prediction_type", "epsilon") == "epsilon":
        assert all(r[:2] == (0.0, 1.0) for r in rows)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, 8, generator=g) * sch.init_noise_sigma
    x0, es, zs = x.clone(), [], []
    for i, t in enumerate(sch.timesteps[first:], start=first):
        with sch.coefficient_walk():
            assert sch.model_input_scale(t) == scales_rows[i][0]
        es.append(torch.randn(2, 4, 8, 8, generator=g))
        zs.append(torch.randn(2, 4, 8, 8, generator=g))
        x = sch.step(es[-1], t, x, noise=zs[-1]).prev_sample if anc else sch.step(es[-1], t, x).prev_sample
        assert x.dtype == torch.float32
    want = _rows_loop(rows[first:], x0.double(), [e.double() for e in es], [z.double() for z in zs])
    scale = max(float(x0.abs().max()), float(want.abs().max()))
    worst = float((x.double() - want).abs().max()) / (16 * 2.0 ** -24 * len(es) * scale)
    print(f"{name:<22} {len(es)} evaluations: |step - rows| / (16 u evaluations max|x|) = {worst:.3f}")
    assert worst < 1.0


@BOTH
def test_coefficient_walk_restores_a_mid_loop_state(anc):
    sch = CLS[anc](**DC.SD)
    sch.set_timesteps(4)
    x = torch.ones(1, 4)
    x = sch.step(0.1 * x, sch.timesteps[0], x).prev_sample     # parked: second order next
    before = (sch.step_index, sch.sample)
    with sch.coefficient_walk():
        row = sch.dpm2_coefficients(sch.timesteps[1])
        assert row[4] == 1.0 and (row[3] > 0.0) == anc and sch.state_in_first_order and sch.step_index == 2
    assert sch.step_index == before[0] and sch.sample is before[1]


def test_ancestral_step_draws_once_per_evaluation_and_noise_planes_give_the_same_bits():
    """the generic ``step`` with a generator, against the same planes drawn ahead and passed as ``noise=``: bit for bit, with the
    generator left in the same state -- 2n - 1 draws for 2n - 1 evaluations, the first-order ones included"""
    kw, steps = dict(DC.SD, prediction_type="v_prediction"), 6
    a, b = KDPM2AncestralDiscreteScheduler(**kw), KDPM2AncestralDiscreteScheduler(**kw)
    a.set_timesteps(steps)
    b.set_timesteps(steps)
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(DC.SHAPE, generator=g) * a.init_noise_sigma
    es = [torch.randn(DC.SHAPE, generator=g) for _ in a.timesteps]
    ga, gb = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    planes = [torch.randn(DC.SHAPE, generator=gb, dtype=torch.float32) for _ in b.timesteps]
    assert len(planes) == 11
    xa = xb = x0
    for t, e, z in zip(a.timesteps, es, planes):
        xa = a.step(e, t, xa, generator=ga).prev_sample
        xb = b.step(e, t, xb, noise=z).prev_sample
        assert torch.equal(xa, xb)
    assert torch.equal(ga.get_state(), gb.get_state())
    # a first-order evaluation draws and does not use: a NaN plane there leaves the latents alone, in a stage 2 it does not
    c = KDPM2AncestralDiscreteScheduler(**kw)
    c.set_timesteps(steps)
    nan = torch.full(DC.SHAPE, float("nan"))
    y = c.step(es[0], c.timesteps[0], x0, noise=nan).prev_sample
    assert torch.isfinite(y).all() and not torch.isfinite(c.step(es[1], c.timesteps[1], y, noise=nan).prev_sample).any()


@BOTH
def test_refusals(anc):
    cls = CLS[anc]
    with pytest.raises(NotImplementedError, match="trained_betas"):
        cls(trained_betas=[0.1, 0.2])
    with pytest.raises(NotImplementedError, match="squaredcos_cap_v2"):
        cls(beta_schedule="squaredcos_cap_v2")
    with pytest.raises(ValueError, match="is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'."):
        cls(timestep_spacing="middle")
    x = torch.ones(1, 4)
    smp = cls(prediction_type="sample")       # constructs, as the reference's does; step refuses
    smp.set_timesteps(4)
    assert torch.equal(smp.scale_model_input(x, smp.timesteps[0]), x / ((torch.tensor(float(smp.sigmas[0])) ** 2 + 1) ** 0.5))
    g = torch.Generator().manual_seed(5)
    state = g.get_state()
    with pytest.raises(NotImplementedError, match="prediction_type not implemented yet: sample"):
        smp.step(x, smp.timesteps[0], x, **(dict(generator=g) if anc else {}))
    assert torch.equal(g.get_state(), state) != anc      # the ancestral reference draws before it refuses
    with pytest.raises(NotImplementedError, match="prediction_type not implemented yet: sample"):
        smp.dpm2_coefficients(smp.timesteps[0])
    bad = cls(prediction_type="velocity")
    bad.set_timesteps(4)
    with pytest.raises(ValueError, match="must be one of `epsilon`, or `v_prediction`"):
        bad.step(x, bad.timesteps[0], x)
    with pytest.raises(ValueError, match="must be one of `epsilon`, or `v_prediction`"):
        bad.dpm2_coefficients(bad.timesteps[0])
