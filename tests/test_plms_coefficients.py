"""PNDMScheduler.plms_coefficients says what PNDMScheduler.step does (skip_prk_steps: PLMS), host side, no GPU.

For every configuration of tests/plms_cases.py the toy loop runs through ``step`` in float64 with every (x, e) pair recorded; the rows
of ``plms_coefficients``, rounded to float32 as the device table holds them, are then applied in float64 to the recorded model outputs
-- the ring of three planes, the parked sample, the slot, all as the header of mi355x_sd_plms_update states them -- and must end where
``step`` ended. The bound is derived here from the float32 rounding of the table alone: a, b, p and q are float32 values already (the
schedule's own numpy expressions), so only the weights that are no float32 numbers (the thirds and twelfths of the longer histories)
contribute, and rows 0 to 2 must agree to float64 roundoff."""
import pytest
import torch

from paddlemix_amd.schedulers import PNDMScheduler
from tests.plms_cases import CONFIGS, PLMS, toy_loop

U64 = 2.0 ** -53


def _rows(sch, ts):
    with sch.coefficient_walk():
        return [sch.plms_coefficients(t) for t in ts]


def _apply(rows, x0, es):
    """the rows (float32 table entries) applied in float64 as the entry's contract states them -> (the latents after every row, the
    bound on their distance from step()'s: the table's rounding carried through the loop, plus the float64 roundings of both sides)"""
    x = x0.clone()
    P, H = torch.full_like(x, float("nan")), torch.full((3,) + tuple(x.shape), float("nan"), dtype=x.dtype)   # never read before written
    E_x, E_P = torch.zeros_like(x), torch.zeros_like(x)
    xs, Es = [], []
    for row, e in zip(rows, es):
        r32 = torch.tensor(row, dtype=torch.float32).double().tolist()
        a, b, p, q = r32[:4]
        slot, park, from_park = int(r32[8]), r32[9] != 0.0, r32[10] != 0.0
        d = [abs(u - v) for u, v in zip(r32[:8], row[:8])]
        assert d[:4] == [0.0] * 4 and row[11] == 0.0   # a, b, p, q: float32 numbers; the pad
        m, dm, mag = r32[4] * e, d[4] * e.abs(), abs(r32[4]) * e.abs()
        for k in (1, 2, 3):
            if r32[4 + k] != 0.0:
                h = H[(slot - k) % 3]
                m, dm, mag = m + r32[4 + k] * h, dm + d[4 + k] * h.abs(), mag + abs(r32[4 + k]) * h.abs()
        S, E_S = (P, E_P) if from_park else (x, E_x)
        if p != 0.0:
            m, dm, mag = p * S + q * m, abs(p) * E_S + abs(q) * dm, abs(p) * S.abs() + abs(q) * mag
        out = a * S + b * m
        # float64: at most 16 roundings on either side (7 in the combination, 3 in the conversion, 3 in the update, step()'s own
        # grouping (1 / 24) * (...) and the float() of its coefficients), each on a partial sum below the absolute sum of the terms
        E_out = abs(a) * E_S + abs(b) * dm + 16 * U64 * (abs(a) * S.abs() + abs(b) * mag)
        if not from_park:
            H[slot] = e
        if park:
            P, E_P = x, E_x
        x, E_x = out, E_out
        xs.append(x)
        Es.append(E_x)
    return xs, Es


@pytest.mark.parametrize("name", list(CONFIGS))
def test_rows_applied_in_float64_equal_step(name):
    kw, steps, first = CONFIGS[name]
    sch = PNDMScheduler(**kw)
    want, es, ts = toy_loop(sch, steps, first)
    # n steps are n + 1 evaluations (the second timestep twice); set_timesteps(1) has nothing to repeat and gives one
    assert len(ts) == (steps + 1 if steps > 1 else 1) - first and want[-1].dtype == torch.float64 and sch.counter == len(ts)
    sch.set_timesteps(steps)
    rows = _rows(sch, ts)
    assert len(rows) == len(ts) and all(len(r) == 12 for r in rows)   # n + 1 rows for n steps; 48 bytes each
    got, E = _apply(rows, want[0], es)
    worst = 0.0
    for i, (g, w, e) in enumerate(zip(got, want[1:], E)):
        err = (g - w).abs()
        assert (err <= e).all(), (name, i, float((err / e).max()))
        worst = max(worst, float((err / e).max()))
    rel = float((E[-1] / want[-1].abs().max()).max())
    print(f"{name}: {len(rows)} rows, worst |rows - step| / bound {worst:.3f}; the bound is at most {rel:.2e} of the latents")
    assert torch.isfinite(got[-1]).all() and rel < 2.0 ** -20   # a bound that is about the table's rounding, not a loose one


def test_the_rows_follow_the_counter_not_the_place_in_the_schedule():
    sch = PNDMScheduler(**PLMS, steps_offset=1)
    sch.set_timesteps(10)
    ts = [int(t) for t in sch.timesteps]
    assert len(ts) == 11 and ts[1] == ts[2]
    whole, tail = _rows(sch, ts), _rows(sch, ts[4:])
    W = PNDMScheduler._PLMS_WEIGHTS
    for rows in (whole, tail):
        assert [r[4:8] for r in rows[:5]] == [W[(0, 1)], W[(1, 1)], W[(2, 2)], W[(3, 3)], W[(4, 4)]]
        assert all(r[4:8] == W[(4, 4)] for r in rows[4:])
        assert [r[8] for r in rows[:7]] == [0.0, 1.0, 1.0, 2.0, 0.0, 1.0, 2.0]              # the ring's slot
        assert [r[9] for r in rows] == [1.0] + [0.0] * (len(rows) - 1)                       # park: the first evaluation alone
        assert [r[10] for r in rows] == [0.0, 1.0] + [0.0] * (len(rows) - 2)                 # from_park: the second alone
        assert all(r[2:4] == (0.0, 1.0) for r in rows)                                       # epsilon: no conversion
    assert whole[7][8] == 0.0 and whole[10][8] == 0.0
    assert sum(W[(4, 4)]) == pytest.approx(1.0) and sum(abs(w) for w in W[(4, 4)]) == pytest.approx(160 / 24)
    # the second evaluation steps from t + step to t, whatever the schedule has there: in the loop from index 4 it repeats the move
    # of its first evaluation (step_plms's own behaviour), where the whole schedule's second row repeats ITS first
    assert tail[1][:2] == tail[0][:2] and whole[1][:2] == whole[0][:2] and tail[0][:2] == whole[4][:2]
    v = PNDMScheduler(**PLMS, prediction_type="v_prediction")
    v.set_timesteps(10)
    rv = _rows(v, v.timesteps)
    assert all(r[2] > 0.0 and r[3] > 0.0 and abs(r[2] ** 2 + r[3] ** 2 - 1.0) < 1e-6 for r in rv)


def test_the_walk_puts_the_state_back():
    sch = PNDMScheduler(**PLMS, steps_offset=1)
    sch.set_timesteps(5)
    assert (sch.counter, sch.ets, sch.cur_sample, sch.cur_model_output) == (0, [], None, 0)
    with sch.coefficient_walk():
        for t in sch.timesteps:
            sch.plms_coefficients(t)
        assert sch.counter == 6 and len(sch.ets) == 4 and sch.cur_sample is None
    assert (sch.counter, sch.ets, sch.cur_sample, sch.cur_model_output) == (0, [], None, 0)
    # and a scheduler that has stepped: the walk cannot continue from tensors the ring never saw, and leaves them alone
    x = torch.zeros(1, 4)
    sch.step(x, sch.timesteps[0], x)
    ets = list(sch.ets)
    with sch.coefficient_walk():
        with pytest.raises(NotImplementedError):
            sch.plms_coefficients(sch.timesteps[1])
    assert sch.counter == 1 and len(sch.ets) == 1 and sch.ets[0] is ets[0] and sch.cur_sample is x


@pytest.mark.parametrize("kw", [dict(skip_prk_steps=False), dict(skip_prk_steps=True, prediction_type="sample")])
def test_what_is_not_fused_is_refused(kw):
    sch = PNDMScheduler(**dict(PLMS, **kw))
    sch.set_timesteps(20)
    with sch.coefficient_walk():
        with pytest.raises(NotImplementedError):
            sch.plms_coefficients(sch.timesteps[0])
    assert sch.counter == 0 and sch.ets == []


def test_a_row_that_is_not_finite_is_refused():
    sch = PNDMScheduler(**PLMS)
    sch.set_timesteps(10)
    sch.alphas_cumprod = sch.alphas_cumprod.copy()
    sch.alphas_cumprod[int(sch.timesteps[0])] = 0.0   # a_t = 0: sqrt(a_prev / a_t) is inf
    with sch.coefficient_walk():
        with pytest.raises(NotImplementedError):
            sch.plms_coefficients(sch.timesteps[0])
    with pytest.raises(ValueError):
        PNDMScheduler(**PLMS).plms_coefficients(1)   # set_timesteps first, as for step
