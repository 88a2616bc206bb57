"""-m gpu: the vectorised rollout of image observations (VectorActor on an image agent: dtqn_img_actor_forward_batch) on the MI355X.
d_model 64, 8 heads, 1 layer, context 6, 4 actions; frames of (3, 32, 32) and (1, 16, 24); N = 3 seeded synthetic environments with
episodes of 2, 5 and 11 steps: ragged prefixes, a context that slides past L so the ring wraps, resets mid-run (image_vector_helpers.py;
the same checks run on the HIP emulation in test_image_vector.py)."""
import numpy as np
import pytest
import torch

import image_vector_helpers as IV

pytestmark = pytest.mark.gpu

SHAPES = [(3, 32, 32), (1, 16, 24)]


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


def make(shape, **kw):
    from dtqn_amd.agents.vector import VectorActor
    agent = IV.make_agent(None, "cuda", shape, **kw)
    return agent, VectorActor(agent, IV.make_envs(shape))


def test_vector_actor_constructs_for_an_image_agent(lib):
    agent, vec = make(SHAPES[0])
    assert vec.image == SHAPES[0] and vec.n == 3
    vec.reset_all()
    q = vec.q_values()
    assert q.shape == (3, IV.A) and np.isfinite(q).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_q_rows_equal_the_module_forward_and_the_oracle_with_frozen_parameters(lib, shape):
    agent, vec = make(shape)
    IV.frozen_run(agent, vec, shape, steps=20)
    assert vec.episodes_done >= 10 + 4 + 1 and vec.max_t >= IV.L


@pytest.mark.parametrize("reload_at", [None, 9])
def test_q_rows_follow_the_parameters_through_updates_and_a_load_state_dict(lib, reload_at):
    agent, vec = make(SHAPES[0])
    IV.training_run(agent, vec, SHAPES[0], steps=20, reload_at=reload_at)


def test_embedding_reuse_on_and_off_agree_and_only_new_frames_are_encoded(lib, monkeypatch):
    monkeypatch.delenv(IV.REUSE_ENV, raising=False)
    agent, vec = make(SHAPES[0])
    q_on, tok_on, fresh_on = IV.frozen_run(agent, vec, SHAPES[0], check=False)
    monkeypatch.setenv(IV.REUSE_ENV, "0")
    agent, vec = make(SHAPES[0])
    q_off, tok_off, fresh_off = IV.frozen_run(agent, vec, SHAPES[0], check=False)
    assert np.array_equal(q_on, q_off)
    assert fresh_on == fresh_off == [3] * 20
    assert tok_on == fresh_on
    assert tok_off[0] == 3 and max(tok_off) == 2 + 5 + 6 and all(t >= f for t, f in zip(tok_off, fresh_off))


def test_dropout_actions_repeat_with_the_seed_and_evaluation_runs_without(lib):
    def run():
        agent, vec = make(SHAPES[0], dropout=0.1)
        vec.reset_all()
        for _ in range(12):
            vec.step_all(0.0)
        return agent, vec, [list(e.taken) for e in vec.envs]
    _, _, a = run()
    agent, vec, b = run()
    assert a == b and all(len(t) == 12 for t in a)
    agent.eval_on()
    vec.reset_all()
    for step in range(8):
        q = vec.q_values().copy()
        assert np.array_equal(q, IV.module_rows(agent, IV.prefixes(vec))), step
        vec.step_all(0.0)
    q_eval = vec.q_values().copy()
    agent.eval_off()
    q_train = vec.q_values().copy()
    assert np.isfinite(q_train).all() and not np.array_equal(q_eval, q_train)        # train mode drops units


def test_replay_after_a_vector_run_is_what_the_single_environment_loop_writes(lib):
    """The device arrays after 40 vector steps against a reference built WITHOUT the actor: fresh environments with the same seeds are
    driven one at a time by the actions the run took (PixelEnv.taken), and every episode goes into the oracle buffer through the
    single-environment loop's calls (store_obs, store per step, flush) in the order the episodes finished (by vector step, then by
    environment).  Wrong frame order, a wrong action or reward, a dropped first observation or mixed-up environments all show."""
    from oracle import replay_oracle as RO
    shape, lengths, steps = SHAPES[0], (2, 5, 11), 40
    agent, vec = make(shape)
    rb, T = agent.replay_buffer, 11
    vec.reset_all()
    for _ in range(steps):
        vec.step_all(0.3)
    assert vec.episodes_done == 20 + 8 + 3 and rb.pos[0] > rb.max_size          # the replay ring wrapped
    taken = [list(e.taken) for e in vec.envs]
    assert all(len(t) == steps for t in taken) and len({tuple(t) for t in taken}) == 3
    shadow = RO.ReplayOracle(rb.max_size * T, int(np.prod(shape)), agent.obs_mask, T, agent.context_len)
    finished = []                                   # (vector step it ended on, environment, first frame, [(frame, action, reward, done)])
    for i, env in enumerate(IV.make_envs(shape, lengths)):
        for k in range(steps // lengths[i]):
            first, rows = env.reset(), []
            for t in range(lengths[i]):
                a = taken[i][k * lengths[i] + t]
                obs, r, done, info = env.step(a)
                rows.append((obs, a, r, done))
            assert done
            finished.append(((k + 1) * lengths[i], i, first, rows))
    for _, _, first, rows in sorted(finished, key=lambda e: (e[0], e[1])):
        shadow.store_obs(first.reshape(-1))
        for t, (obs, a, r, done) in enumerate(rows):
            shadow.store(obs.reshape(-1), a, r, done, t + 1)
        shadow.flush()
    arrays = rb.export_arrays()
    assert arrays["obss"].dtype == np.uint8
    assert np.array_equal(arrays["obss"].reshape(shadow.obss.shape), shadow.obss.astype(np.uint8))
    assert np.array_equal(arrays["actions"], shadow.actions[:, :, 0])
    assert np.array_equal(arrays["rewards"], shadow.rewards[:, :, 0])
    assert np.array_equal(arrays["dones"].astype(bool), shadow.dones[:, :, 0])
    assert np.array_equal(rb.dev.ep_len.cpu().numpy(), shadow.episode_lengths) and list(rb.pos) == list(shadow.pos)


def test_run_py_with_num_envs_on_a_pixel_environment(lib, monkeypatch, tmp_path):
    """run.py --num-envs 3 end to end: prepopulate, train (vector steps with their updates queued behind the actor), evaluate."""
    import run as runpy
    from dtqn_amd import envs as E
    monkeypatch.setitem(E.REGISTRY, "SyntheticPixels-v0", lambda: IV.PixelEnv((3, 32, 32), 7, 5))
    monkeypatch.chdir(tmp_path)
    args = runpy.get_args(("--envs SyntheticPixels-v0 --num-envs 3 --num-steps 24 --prepopulate 60 --batch 2 --context 6 --history 6 "
                           "--in-embed 64 --heads 8 --layers 1 --buf-size 400 --eval-frequency 12 --eval-episodes 1 --disable-wandb "
                           "--sampler device").split())
    agent = runpy.run_experiment(args)
    assert agent.image == (3, 32, 32) and agent.num_train_steps == 24 and np.isfinite(agent.td_errors.mean())
