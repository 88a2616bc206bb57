"""Device-resident greedy evaluation of a bag network: `DeviceEvaluator` with the persistent-memory bag of every evaluation environment
kept, filled and chosen on the GPU.

`DeviceEvaluator` (device_eval.py) refuses a bag agent: its vector step knows nothing of bags, and the host paths (`run.evaluate`,
`VectorEvaluator`) pay one module forward per environment step plus one over K + 1 candidate bags and a blocking read per choice.
`DeviceBagEvaluator` is that evaluator with the bag state of `DeviceBagVectorActor` (device_bag.py, csrc/dtqn_devbag.hip) in a second
allocation.  A vector step is `dtqn_deval_step_bag`: the eval-mode forward with the bags, the evaluation's step kernel, the bags'
bookkeeping kernel pointed at the evaluation's state -- an episode that finished clears its bag, an idle environment does nothing -- and
on the steps where a choice can be due the candidate forward and the selection.  The candidate forward is
`dtqn_forward_bag_candidates`: the K + 1 candidates of an environment share its one context and the bag enters the network behind the
layers, so embedding and layers run once per environment and only the bag branch and the head per candidate.

`may_choose` is the host's, by the rollout's rule (device_bag.py), counted in vector steps since `begin`.  Everything `DeviceEvaluator`
promises holds, bag choices included: exactly `episodes` episodes, each a function of (seed, key, episode index) alone -- an episode's
bag starts cleared and sees only that episode's evictions -- a key that is never repeated, and nothing of the agent moved.  Dropout
networks are admitted: the evaluation never runs train mode."""
from __future__ import annotations

from .device_bag import DeviceBags
from .device_eval import DeviceEvaluator


class DeviceBagEvaluator(DeviceBags, DeviceEvaluator):
    def _refuse(self, agent) -> None:
        if agent.bag.size < 1:
            raise ValueError("DeviceBagEvaluator is the device-resident evaluation of a bag network (--bag-size K > 0); without a bag: "
                             "DeviceEvaluator")
        super()._refuse(agent)

    def _alloc_state(self, desc) -> None:
        """The evaluation's state, then the bags' (the workspace is the shared-trunk candidate forward's)."""
        super()._alloc_state(desc)
        eng = self.agent.engine
        self._alloc_bags(desc, eng.lib.dtqn_bag_candidates_workspace_floats(eng._actor_net_ref, self.n, self.agent.bag.size + 1))

    def _call(self, name: str, *more) -> None:
        """The evaluation's entry points; `begin` is the bag path's (get_state and set_state serve both)."""
        if name != "begin":
            return super()._call(name, *more)
        lib, net = self._lib_args()
        self._check(lib.dtqn_deval_begin_bag(net, self._ev_ref, self._bag_ref, *more, self.agent.engine._stream()), "dtqn_deval_begin_bag")
        self._restart_choice_clock()

    def step(self) -> None:
        """One vector step of the evaluation in progress, enqueued: up to five launches."""
        agent = self.agent
        lib, net = self._lib_args()
        self._throttle()
        n_max = self.next_n_max()
        may_choose = self._may_choose()
        rc = lib.dtqn_deval_step_bag(net, agent._theta_p, self._ev_ref, self._bag_ref, self.key, self._step & 0xFFFFFFFF, self._cur, n_max,
                                     self.episodes, 1 if may_choose else 0, agent.engine._stream())
        self._check(rc, "dtqn_deval_step_bag")
        self._pending = True
        self._issue()
        self._step += 1
        self._count_step(may_choose)
