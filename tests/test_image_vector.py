"""Vectorised rollout of image observations on the test-only HIP emulation: (1, 8, 8) frames, N = 2 environments with episodes of 2 and
11 steps (ragged prefixes, a context that slides past L = 6 so the ring wraps, resets mid-run).  The same checks run on the MI355X at
the sizes of test_gpu_image_vector.py."""
import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B

import image_vector_helpers as IV

SHAPE, LENGTHS = (1, 8, 8), (2, 11)


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


def make(emu, shape=SHAPE, **kw):
    from dtqn_amd.agents.vector import VectorActor
    agent = IV.make_agent(emu, "cpu", shape, **kw)
    return agent, VectorActor(agent, IV.make_envs(shape, LENGTHS))


def test_q_rows_equal_the_module_forward_and_the_oracle_with_frozen_parameters(emu):
    agent, vec = make(emu)
    qs, tokens, fresh = IV.frozen_run(agent, vec, SHAPE, steps=12)       # (the emulation is slow: 12 steps reach every case the 20 on the GPU do)
    assert vec.episodes_done >= 6 + 1 and vec.max_t >= IV.L       # resets happened, the ring wrapped


def test_q_rows_follow_the_parameters_through_updates_and_a_load_state_dict(emu):
    agent, vec = make(emu)
    IV.training_run(agent, vec, SHAPE, steps=6, reload_at=3)             # an update behind every vector step but one: a load_state_dict alone


def test_embedding_reuse_on_and_off_agree_and_only_new_frames_are_encoded(emu, monkeypatch):
    monkeypatch.delenv(IV.REUSE_ENV, raising=False)
    agent, vec = make(emu)
    q_on, tok_on, fresh_on = IV.frozen_run(agent, vec, SHAPE, steps=10, check=False)
    monkeypatch.setenv(IV.REUSE_ENV, "0")
    agent, vec = make(emu)
    q_off, tok_off, fresh_off = IV.frozen_run(agent, vec, SHAPE, steps=10, check=False)
    assert np.array_equal(q_on, q_off)
    assert fresh_on == fresh_off == [len(LENGTHS)] * len(fresh_on)
    assert tok_on == fresh_on                                    # (step 0: every window is one new frame)
    assert tok_off[0] == len(LENGTHS) and max(tok_off) > len(LENGTHS) and all(t >= f for t, f in zip(tok_off, fresh_off))


@pytest.mark.parametrize("shape", [SHAPE, (1, 9, 9)])       # 81 bytes: no multiple of 16, the ring push goes byte by byte
def test_host_bookkeeping_against_a_list_of_frames(emu, shape):
    """head / len / valid across resets and wrap-around: the frame ring and the embedding marks against a plain list-of-frames model.
    The steps in between explore in every environment, so their frames reach the ring through push-only launches and their embeddings
    are made by the next full one; Q of that launch equals the module forward bit for bit."""
    agent, vec = make(emu, shape)
    vec.reset_all()
    N, L, O = vec.n, vec.L, int(np.prod(shape))
    for step in range(12):
        q = vec.q_values().copy()
        if step % 5 == 0:
            IV.check_step(agent, vec, shape, q, ("push-only", step), oracle=False)
        ring = vec._frame_ring.view(N, L, O).numpy()
        for i, p in enumerate(IV.prefixes(vec)):
            t = vec.contexts[i].timestep
            assert vec._len_np[i] == len(p) == min(L, t + 1) and vec._head_np[i] == t % L
            for r in range(len(p)):
                assert np.array_equal(ring[i, (t - (len(p) - 1) + r) % L], p[r].reshape(-1)), (step, i, r)
            assert vec._valid[i, :len(p)].all() and not vec._valid[i, len(p):].any()
        calls = agent._actor_calls
        vec.step_all(1.0)                # all-random actions, twice: the second launch carries the frame of the first step, push only
        vec.step_all(1.0)
        assert agent._actor_calls == calls and agent.engine.lib.dtqn_debug_last_img_actor_tokens() == 0


def test_a_frame_of_another_dtype_is_refused(emu):
    from dtqn_amd.agents.vector import VectorActor
    agent = IV.make_agent(emu, "cpu", SHAPE)
    envs = IV.make_envs(SHAPE, LENGTHS)
    envs[1].observation_space.dtype = np.float32
    with pytest.raises(TypeError):
        VectorActor(agent, envs)
