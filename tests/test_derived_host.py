"""ams_hip/ops.py::derived checked on the CPU: the one cache and the one staleness rule of everything derived from weight tensors, and the
frozen mark it reads -- set and cleared through one setter, never left on a variable an optimizer writes."""
import pytest

torch = pytest.importorskip('torch')

from ams_hip import ops
from ams_hip._lib import AmsError


@pytest.fixture
def next_pass(monkeypatch):
    monkeypatch.setattr(ops, 'PASS', [ops.PASS[0]])          # the counter of these tests alone

    def bump():
        ops.PASS[0] += 1
    return bump


class Maker(object):
    """make() of a derived value: counts its calls, remembers what it was handed, returns a new tensor each time."""

    def __init__(self):
        self.calls, self.olds = 0, []

    def __call__(self, old):
        self.calls += 1
        self.olds.append(old)
        return torch.full((1,), float(self.calls))


def test_kept_within_a_pass_and_remade_in_the_next(next_pass):
    w, make = torch.zeros(3), Maker()
    a = ops.derived((w,), 'x', make)
    assert ops.derived((w,), 'x', make) is a and make.calls == 1
    assert ops.derived(w, 'x', make) is a and make.calls == 1            # one owner may be given bare
    next_pass()
    b = ops.derived((w,), 'x', make)
    assert b is not a and make.calls == 2 and ops.derived_entry(w, 'x') is b
    assert ops.derived((w,), 'y', make) is not b and make.calls == 3     # names do not share a slot
    assert ops.derived((w,), 'x', make) is b


def test_kept_across_passes_only_when_every_owner_is_frozen(next_pass):
    w, v, make = torch.zeros(3), torch.zeros(3), Maker()
    ops.set_frozen(w, True)
    a = ops.derived((w, v), 'x', make)
    next_pass()
    b = ops.derived((w, v), 'x', make)                                   # only the first owner is frozen
    assert b is not a and make.calls == 2
    ops.set_frozen(w, False)
    ops.set_frozen(v, True)
    a = ops.derived((w, v), 'x', make)
    next_pass()
    b = ops.derived((w, v), 'x', make)                                   # only the second owner is frozen
    assert b is not a and make.calls == 4
    ops.set_frozen(w, True)
    a = ops.derived((w, v), 'x', make)
    for _ in range(3):
        next_pass()
        assert ops.derived((w, v), 'x', make) is a
    assert make.calls == 5


def test_remade_on_a_changed_key_and_on_a_changed_second_owner(next_pass):
    w, v, v2, make = torch.zeros(3), torch.zeros(3), torch.zeros(3), Maker()
    for t in (w, v, v2):
        ops.set_frozen(t, True)
    a = ops.derived((w, v), 'x', make, key=(4, torch.Size((2, 3)), 7))
    assert ops.derived((w, v), 'x', make, key=(4, torch.Size((2, 3)), 7)) is a
    assert ops.derived((w, v), 'x', make, key=(4, (2, 3), 7)) is a
    b = ops.derived((w, v), 'x', make, key=(5, (2, 3), 7))
    assert b is not a and make.calls == 2
    c = ops.derived((w, v), 'x', make, key=(5, (2, 3), 8))
    assert c is not b and make.calls == 3
    d = ops.derived((w, v2), 'x', make, key=(5, (2, 3), 8))              # v2 == v elementwise: owners are compared by identity
    assert d is not c and make.calls == 4
    assert ops.derived((w,), 'x', make, key=(5, (2, 3), 8)) is not d and make.calls == 5
    next_pass()
    assert ops.derived((w,), 'x', make, key=(5, (2, 3), 8)) is ops.derived_entry(w, 'x') and make.calls == 5


def test_make_receives_the_old_value_and_may_refresh_it_in_place(next_pass):
    w, make = torch.zeros(3), Maker()
    a = ops.derived((w,), 'x', make)
    next_pass()
    b = ops.derived((w,), 'x', make)
    assert make.olds[0] is None and make.olds[1] is a
    w = torch.tensor([1.0, -3.0, 2.0])

    def bound(old):                                                      # the form of the operand bounds: same tensor, new value
        out = torch.empty(1) if old is None else old
        return out.copy_(w.abs().max().reshape(1))
    first = ops.derived((w,), 'amax', bound)
    assert float(first) == 3.0
    w.mul_(2.0)
    assert float(ops.derived((w,), 'amax', bound)) == 3.0                # this pass: not measured again
    next_pass()
    again = ops.derived((w,), 'amax', bound)
    assert again is first and again.data_ptr() == first.data_ptr() and float(first) == 6.0


def test_keep_frozen_stores_nothing_for_unfrozen_owners(next_pass):
    w, v, make = torch.zeros(3), torch.zeros(3), Maker()
    a = ops.derived((w, v), 'x', make, keep='frozen')
    b = ops.derived((w, v), 'x', make, keep='frozen')
    assert a is not b and make.calls == 2 and make.olds == [None, None]
    assert ops.derived_entry(w, 'x') is None and not hasattr(w, '_ams_derived')
    ops.set_frozen(w, True)
    ops.derived((w, v), 'x', make, keep='frozen')
    assert ops.derived_entry(w, 'x') is None                             # v is not frozen
    ops.set_frozen(v, True)
    c = ops.derived((w, v), 'x', make, keep='frozen')
    next_pass()
    assert ops.derived((w, v), 'x', make, keep='frozen') is c and ops.derived_entry(w, 'x') is c and make.calls == 4


def test_setting_and_clearing_the_frozen_mark_drop_what_was_derived(next_pass):
    w, make = torch.zeros(3), Maker()
    ops.derived((w,), 'x', make)
    ops.set_frozen(w, True)
    assert ops._frozen(w) and ops.derived_entry(w, 'x') is None and not hasattr(w, '_ams_derived')
    a = ops.derived((w,), 'x', make)
    next_pass()
    assert ops.derived((w,), 'x', make) is a
    ops.set_frozen(w, False)
    assert not ops._frozen(w) and ops.derived_entry(w, 'x') is None and not hasattr(w, '_ams_derived')
    assert ops.derived((w,), 'x', make) is not a and make.olds[-1] is None
    ops.set_frozen(w, False)                                             # clearing an unset mark is not an error
    ops.derived((w,), 'x', make)
    ops.drop_frozen_derivatives(w)
    assert ops.derived_entry(w, 'x') is None


def test_freeze_then_train_leaves_no_trained_variable_frozen(tmp_path):
    """freeze_weights() marks every variable; optimize() must clear the mark (and what was derived under it) on the variables it trains
    before the optimizer takes them, and leaves the others frozen."""
    from tests.smoke_step import build_front_dpcl
    trainer, tfds = build_front_dpcl(str(tmp_path), B=2, L=256, W=32, N=8, hop=8, layer_size=8, nb_layers=2, E=4)
    g, model = trainer.graph, trainer.model
    with g.as_default():
        model.freeze_weights()
        assert all(ops._frozen(v) for v in g.variables.values())
        for v in model.trainable_variables:
            ops.derived((v,), 'x', lambda old: torch.zeros(1))
        del model._cache_optimize                                        # (the recipe built its optimizer during construction)
        opt = model.optimize
    trained = set(id(v) for v in model.trainable_variables)
    assert len(trained) == 2 * 2 * 2 + 2 and opt.vars == list(model.trainable_variables)
    for v in g.variables.values():
        if id(v) in trained:
            assert not ops._frozen(v) and not hasattr(v, '_ams_derived'), v.ams_name
        else:
            assert ops._frozen(v), v.ams_name


def test_flat_optimizer_refuses_a_frozen_parameter():
    from ams_hip.optim import FlatOptimizer
    a, b = torch.zeros(4, 3, requires_grad=True), torch.zeros(5, requires_grad=True)
    ops.set_frozen(b, True)
    with pytest.raises(AmsError):
        FlatOptimizer([a, b], 'Adam', 1e-3, 10, 200.0)
    ops.set_frozen(b, False)
    opt = FlatOptimizer([a, b], 'Adam', 1e-3, 10, 200.0)
    assert opt.flat.numel() == 17
