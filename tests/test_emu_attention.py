"""Attention capture (DTQN(..., capture_attention=True), dtqn_attn_weights) on the CPU emulation of the HIP sources: every layer's
head-averaged causal attention weights and the bag weights against the reference's own (G13), and what capture must leave alone --
Q bit for bit, gradients, state_dict keys -- plus the refusals."""
import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B
from dtqn_amd.networks.dtqn import DTQN
from oracle import dtqn_oracle as O

from attention_helpers import capture_module, captured, check_weights, g13, g13_case, g13_names, tensors
from autograd_helpers import hip_grads, make_inputs, make_module


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.fixture(scope="module")
def z():
    with g13() as f:
        yield {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", g13_names())
def test_weights_match_the_reference(emu, z, name):
    cfg, params, inputs, q_ref, ref_alphas, ref_bag = g13_case(z, name)
    m = capture_module(emu, cfg, params)
    q = m(**tensors(inputs)).numpy()
    assert np.abs(q - q_ref).max() <= 1e-4 * max(1.0, float(np.abs(q_ref).max()))
    alphas, bag = captured(m)
    check_weights(alphas, bag, ref_alphas, ref_bag, f64=(cfg, params, inputs))
    assert m.bag_attn_weights is None                      # the reference declares it and never writes it (dtqn.py:135)
    # Q with capture on is the forward with capture off, bit for bit; a second capture gives the same bits
    m.set_capture_attention(False)
    assert torch.equal(torch.as_tensor(q), m(**tensors(inputs)))
    m.set_capture_attention(True)
    m(**tensors(inputs))
    again, bag2 = captured(m)
    for a, b in zip(alphas, again):
        assert np.array_equal(a, b)
    if bag is not None:
        assert np.array_equal(bag, bag2)


def test_alpha_is_none_before_the_first_capture_and_layers_index_like_the_reference(emu, z):
    cfg, params, inputs, _, _, _ = g13_case(z, "cfg1")
    m = make_module(emu, cfg, params, autograd=False)
    assert len(m.transformer_layers) == cfg.num_layers
    assert m.transformer_layers[-1] is m.transformer_layers[cfg.num_layers - 1]
    assert all(layer.alpha is None for layer in m.transformer_layers) and m.bag_attn_weights is None
    m.eval()
    m(**tensors(inputs))                                   # capture off: nothing stored
    assert all(layer.alpha is None for layer in m.transformer_layers)
    m.set_capture_attention(True)
    m(**tensors(inputs))
    n = inputs["obss"].shape[1]
    for layer in m.transformer_layers:
        assert layer.alpha.shape == (inputs["obss"].shape[0], n, n) and layer.alpha.dtype == torch.float32
        assert not layer.alpha.requires_grad


@pytest.mark.parametrize("name", ["cfg1", "bag4", "padded_48_6"])
def test_state_dict_and_parameters_unchanged(emu, z, name):
    cfg, params, inputs, _, _, _ = g13_case(z, name)
    m = make_module(emu, cfg, params, autograd=False)
    keys, plist = list(m.state_dict().keys()), [p.data_ptr() for p in m.parameters()]
    m.set_capture_attention(True).eval()
    m(**tensors(inputs))
    assert list(m.state_dict().keys()) == keys == O.state_dict_keys(cfg)
    assert [p.data_ptr() for p in m.parameters()] == plist


@pytest.mark.parametrize("name", ["prefix", "bag4", "padded_48_6"])
def test_autograd_with_capture(emu, z, name):
    """An autograd forward with capture on stores the same weights as a no-grad capture, and its gradients are those of autograd alone."""
    cfg, params, inputs, _, ref_alphas, ref_bag = g13_case(z, name)
    m = make_module(emu, cfg, params, autograd=True)
    m.eval()
    n = inputs["obss"].shape[1]
    obs, act = inputs["obss"], inputs["actions"]
    bag = (inputs["bag_obss"], inputs["bag_actions"]) if cfg.bag_size > 0 else None
    w = np.random.default_rng(3).standard_normal((obs.shape[0], n, cfg.num_actions)).astype(np.float32)
    q0, g0, d0 = hip_grads(m, obs, act, bag, w)
    m.set_capture_attention(True)
    q1, g1, d1 = hip_grads(m, obs, act, bag, w)
    assert np.array_equal(q0, q1) and np.array_equal(g0, g1) and np.array_equal(d0, d1)
    alphas, bagw = captured(m)
    check_weights(alphas, bagw, ref_alphas, ref_bag, f64=(cfg, params, inputs))
    with torch.no_grad():
        m(**tensors(inputs))
    nograd, bag2 = captured(m)
    for a, b in zip(alphas, nograd):
        assert np.array_equal(a, b)
    if bagw is not None:
        assert np.array_equal(bagw, bag2)


def test_image_networks_are_refused(emu):
    m = DTQN((1, 24, 24), 3, 8, 0, 64, 8, 1, 4, capture_attention=True, _test_lib=emu)
    m._allow_cpu = True
    m.eval()
    with pytest.raises(NotImplementedError, match="attention capture"):
        m(torch.zeros(1, 2, 1, 24, 24, dtype=torch.uint8), torch.zeros(1, 2, 1, dtype=torch.long))


def test_train_mode_dropout_is_refused(emu):
    cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=4, num_layers=1, history_len=20, dropout=0.1)
    m = make_module(emu, cfg, O.init_params(cfg, seed=1, perturb=True), autograd=False)
    m.set_capture_attention(True)
    obs, act, _, _ = make_inputs(cfg, 2, 10, seed=1)
    o, a = torch.as_tensor(obs), torch.as_tensor(act)
    m.train()
    with pytest.raises(NotImplementedError, match="attention capture"):
        m(o, a)
    m.eval()
    with pytest.raises(NotImplementedError, match="attention capture"):
        m(o, a, _train_dropout=(1, 2))                     # the agent's train-mode forwards
    m(o, a)                                                # eval mode: no dropout, captured
    assert m.transformer_layers[0].alpha.shape == (2, 10, 10)
