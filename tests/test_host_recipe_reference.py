"""Pins tests/recipe_reference.py, the plain-torch statement of the whole training recipe that the GPU tests of
tests/test_gpu_full_recipe.py are compared with (no GPU needed): without dropout and on hand-given batches it is the loop
anybody would write, its masks are `dropout.expected_keep`'s, and the chosen seeds meet the input condition under which a
float32 Adam trajectory can be compared with a float64 one at all."""
import pytest
import torch
import torch.nn.functional as F

from dctn_amd import batches, dropout
from oracle import ref_cpu as R
from tests import recipe_reference as RR

CASE_NAMES = list(RR.CASES)


def _hand_batches(case, count, dtype):
    g = torch.Generator().manual_seed(77)
    out = []
    for _ in range(count):
        u = torch.rand(1, 5, case.image_size, case.image_size, generator=g, dtype=torch.float64)
        x = torch.stack((torch.sin(u * torch.pi / 2) ** 2, torch.cos(u * torch.pi / 2) ** 2), dim=-1).to(dtype)
        out.append((x, torch.randint(0, 10, (5,), generator=g)))
    return out


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_without_dropout_on_hand_given_batches_it_is_the_direct_torch_loop(name, dtype):
    case = RR.CASES[name]
    w0 = RR.initial_parameters(case, torch.float32)
    hand = _hand_batches(case, 3, dtype)
    got = RR.run_recipe(w0, dtype=dtype, n=3, p=1.0, dropout_seed=case.dropout_seed, lr=case.lr,
                        weight_decay=case.weight_decay, reg=case.reg, reg_coeff=case.reg_coeff, hand_batches=hand)
    params = [torch.nn.Parameter(t.clone().to(dtype)) for t in w0]
    opt = torch.optim.Adam(params, lr=case.lr, weight_decay=case.weight_decay)
    for k, (x, y) in enumerate(hand):
        *cores, weight, bias = params
        loss = F.cross_entropy(R.eps_plus_linear_forward(cores, weight, bias, x), y)
        if case.reg == "epswise":
            term = (weight ** 2).sum() + sum((c ** 2).sum() for c in cores)
        else:
            term = (weight ** 2).sum() + R.epses_inner_product(cores, cores)
        opt.zero_grad()
        (loss + term * case.reg_coeff).backward()
        opt.step()
        assert got[k]["loss"] == float(loss.detach()) and got[k]["reg_term"] == float(term.detach())
        assert got[k]["indices"] is None
        for a, b in zip(got[k]["params"], params):
            assert a.dtype == dtype and torch.equal(a, b.detach())
    assert not torch.equal(got[0]["params"][0], got[2]["params"][0])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_masks_are_expected_keeps_and_a_dropped_component_sees_the_regulariser_only(name):
    case = RR.CASES[name]
    w0 = RR.initial_parameters(case, torch.float32)
    kept = total = 0
    for draw in (0, 6):
        for s, core in enumerate(w0[:-2]):
            mask = RR.keep_mask(case.dropout_seed, draw, s, core.shape, RR.P_KEEP, torch.float64)
            want = dropout.expected_keep(case.dropout_seed, draw, s, core.numel(), RR.P_KEEP)
            assert mask.shape == core.shape and mask.reshape(-1).tolist() == [float(k) for k in want]
            kept, total = kept + int(mask.sum()), total + core.numel()
    # a binomial(total, 3/4) count: five standard deviations
    assert abs(kept - RR.P_KEEP * total) <= 5 * (total * RR.P_KEEP * (1 - RR.P_KEEP)) ** 0.5
    assert dropout.keep_threshold(RR.P_KEEP) == 3 << 30
    # iteration 0 of the reference: where a component is dropped, the loss has no gradient; Adam sees the regulariser's
    # and the weight decay's, and the kept ones see more than that
    hist = RR.run_case(case, torch.float64, n=1)
    w64 = [t.double() for t in w0]
    cores = [c.clone().requires_grad_(True) for c in w64[:-2]]
    (RR.regulariser(case.reg, cores, w64[-2]) * case.reg_coeff).backward()
    for s, c in enumerate(cores):
        mask = RR.keep_mask(case.dropout_seed, 0, s, c.shape, RR.P_KEEP, torch.float64)
        only_reg = c.grad + case.weight_decay * c.detach()
        seen = hist[0]["adam_grads"][s]
        assert torch.allclose(seen[mask == 0], only_reg[mask == 0], rtol=1e-12, atol=0)
        assert not torch.allclose(seen[mask == 1], only_reg[mask == 1], rtol=1e-3, atol=0)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_batches_are_the_sources_indices_through_the_feature_map(name):
    case = RR.CASES[name]
    images, labels = RR.make_data(case)
    hist = RR.run_case(case, torch.float64, n=5)
    seen = [h["indices"] for h in hist]
    assert seen == [batches.expected_indices(case.batch_seed, k, RR.N_SAMPLES, RR.GLOBAL_BATCH) for k in range(5)]
    assert len(set(sum(seen[:4], []))) == 32 and seen[4] == batches.order(case.batch_seed, 1, RR.N_SAMPLES)[:8]
    # two shards are the two halves of the global batch
    halves = [batches.expected_indices(case.batch_seed, 5, RR.N_SAMPLES, RR.GLOBAL_BATCH, r, 2) for r in range(2)]
    assert halves[0] + halves[1] == batches.expected_indices(case.batch_seed, 5, RR.N_SAMPLES, RR.GLOBAL_BATCH)
    # the float32 batch is the source's table (`batches.feature_table`: the float32 ops once per intensity) looked up
    x32, y = RR.make_batch(images, labels, seen[0], torch.float32, case.scale)
    table = batches.feature_table(RR.PHI, case.scale, torch.float32)
    assert x32.shape == (1, 8, case.image_size, case.image_size, 2) and y.tolist() == labels[seen[0]].tolist()
    assert float((x32 - table[images[seen[0]].long()].unsqueeze(0)).abs().max()) <= 2e-6 * 2 * case.scale
    x64, _ = RR.make_batch(images, labels, seen[0], torch.float64, case.scale)
    assert x64.dtype == torch.float64 and float((x64 - x32.double()).abs().max()) <= 2e-6 * 2 * case.scale
    xb, _ = RR.make_batch(images, labels, seen[0], torch.bfloat16, case.scale)
    assert torch.equal(xb, x32.to(torch.bfloat16))


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("start", [torch.float32, torch.bfloat16], ids=["f32_start", "bf16_start"])
def test_input_condition_no_first_gradient_component_is_rounding_noise(name, start):
    """Adam turns a gradient component that is almost zero into a step of +-lr whose sign is rounding noise.  For the
    seeds of `CASES` no component of what Adam sees in iteration 0 of the float64 reference is below 1e-6 of the
    largest - from the float32 initial values (the float32 tests) and from the bfloat16 ones (the master-weight tests)."""
    case = RR.CASES[name]
    hist = RR.run_case(case, torch.float64, n=1, params_dtype=start)
    g = RR.flat(hist[0]["adam_grads"]).abs()
    print(f"\n{name} {start}: smallest |g| = {float(g.min()):.3e}, largest = {float(g.max()):.3e}, "
          f"ratio {float(g.min() / g.max()):.3e}")
    assert float(g.min()) >= 1e-6 * float(g.max())


def test_the_mixed_precision_form_keeps_float32_masters_and_rounded_parameters():
    case = RR.CASES["cfg2"]
    hist = RR.run_case(case, torch.bfloat16, n=2, master_dtype=torch.float32)
    for h in hist:
        assert all(m.dtype == torch.float32 for m in h["masters"]) and all(p.dtype == torch.bfloat16 for p in h["params"])
        assert all(torch.equal(p, m.to(torch.bfloat16)) for p, m in zip(h["params"], h["masters"]))
    w0 = RR.initial_parameters(case, torch.bfloat16)
    assert not torch.equal(hist[1]["masters"][0], w0[0].float())
