"""variational_cvi_sde._Ahead with records of kind PAIR (the whole first factorisation of the next step, made together with the ELBO's
by Plan.cq_factor_pair), driven without a GPU like test_host_logic.test_record_ahead_bookkeeping: CPU site tensors, stand-ins for the
plan (an epoch) and the structured state (site_sym, version)."""
from types import SimpleNamespace

import numpy as np
import torch


def _setup():
    from vidp_amd.variational_cvi_sde import _Ahead
    plan = SimpleNamespace(epoch=0)
    cq = SimpleNamespace(site_sym=torch.full((3,), 2.0, dtype=torch.float64), version=0)
    site = SimpleNamespace(lin=torch.ones((4, 2), dtype=torch.float64))
    calls = []

    def launch(lin, sym, lr):       # the blend towards a zero gradient, then "the two factorisations"
        lin.copy_((1 - lr) * site.lin)
        sym.copy_((1 - lr) * cq.site_sym)
        plan.epoch += 1
        calls.append(lr)
        return "factor", dict(L="L2 of call %d" % len(calls), y="y2")

    def update(ahead, lr):          # what update_data_sites does with the answer
        got = ahead.accept(lr, site.lin, cq, plan)
        if got is not None:
            site.lin, cq.site_sym = got
        return got

    return _Ahead(), plan, cq, site, calls, launch, update


def test_pair_record_made_accepted_taken():
    ahead, plan, cq, site, calls, launch, update = _setup()
    PAIR, REDUCE = ahead.PAIR, ahead.REDUCE
    assert update(ahead, 0.5) is None and ahead.lr == 0.5
    # made: the first result is handed back, the second factorisation is held
    assert ahead.make(site.lin, cq, plan, launch, kind=PAIR) == "factor" and calls == [0.5]
    assert ahead.rec is not None and ahead.kind == PAIR and ahead.held["L"] == "L2 of call 1"
    # not armed before update_data_sites has taken the prediction over: refused, dropped
    assert ahead.take(site.lin, cq, plan, kind=PAIR) is False and ahead.rec is None and ahead.held is None
    # accepted: the site buffers are exchanged; taken exactly once, and what is taken is the held factorisation
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    old, spare = (site.lin, cq.site_sym), tuple(ahead.bufs)
    assert update(ahead, 0.5) is not None and ahead.consumed == 1
    assert site.lin is spare[0] and cq.site_sym is spare[1] and ahead.bufs[0] is old[0] and ahead.bufs[1] is old[1]
    np.testing.assert_array_equal(site.lin.numpy(), np.full((4, 2), 0.5))
    got = ahead.take(site.lin, cq, plan, kind=PAIR)
    assert got == dict(L="L2 of call 2", y="y2")
    assert ahead.take(site.lin, cq, plan, kind=PAIR) is False and ahead.rec is None and ahead.held is None
    # a record is handed out only as the kind it was made as, either way round
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    assert update(ahead, 0.5) is not None
    assert ahead.take(site.lin, cq, plan) is False and ahead.rec is None and ahead.held is None        # asked for a REDUCE record
    ahead.make(site.lin, cq, plan, lambda *a: launch(*a)[0])                                            # a REDUCE record, as before
    assert ahead.kind == REDUCE and ahead.held is None
    assert update(ahead, 0.5) is not None
    assert ahead.take(site.lin, cq, plan, kind=PAIR) is False and ahead.rec is None


def test_pair_record_refused():
    ahead, plan, cq, site, calls, launch, update = _setup()
    PAIR = ahead.PAIR
    from vidp_amd.stamps import wrote
    assert update(ahead, 0.5) is None
    # another learning rate
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    assert update(ahead, 0.3) is None and ahead.rec is None and ahead.held is None and ahead.consumed == 0
    assert ahead.take(site.lin, cq, plan, kind=PAIR) is False
    assert update(ahead, 0.5) is None
    # a site written by hand after the record was made
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    wrote(site.lin)
    assert update(ahead, 0.5) is None and ahead.rec is None and ahead.held is None and ahead.consumed == 0
    # ... or between accept and take
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    assert update(ahead, 0.5) is not None and ahead.consumed == 1
    wrote(cq.site_sym)
    assert ahead.take(site.lin, cq, plan, kind=PAIR) is False and ahead.rec is None and ahead.held is None
    # a Girsanov update (cq.version) after the record was made / between accept and take
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    cq.version += 1
    assert update(ahead, 0.5) is None and ahead.rec is None and ahead.consumed == 1
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    assert update(ahead, 0.5) is not None and ahead.consumed == 2
    cq.version += 1
    assert ahead.take(site.lin, cq, plan, kind=PAIR) is False and ahead.held is None
    # another factorisation on the plan (plan.epoch) after the record was made / between accept and take
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    plan.epoch += 1
    assert update(ahead, 0.5) is None and ahead.rec is None and ahead.consumed == 2
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    assert update(ahead, 0.5) is not None and ahead.consumed == 3
    plan.epoch += 1
    assert ahead.take(site.lin, cq, plan, kind=PAIR) is False and ahead.rec is None and ahead.held is None
    # drop
    ahead.make(site.lin, cq, plan, launch, kind=PAIR)
    assert ahead.rec is not None and ahead.held is not None
    ahead.drop()
    assert ahead.rec is None and ahead.held is None
    assert update(ahead, 0.5) is None and ahead.take(site.lin, cq, plan, kind=PAIR) is False
    ahead.drop()                                                   # nothing to drop
