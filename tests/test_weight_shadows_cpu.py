"""CPU: the table of bf16 weight shadows (``ops._WeightShadows``) survives parameters that die while it is being rebuilt.

The entries hold weak references.  Every caller drops dead entries before it rebuilds the table, but a garbage collection can
start at any allocation inside the rebuild and free a model whose last references were cyclic (a test module's model after its
fixture was torn down): the rebuild then met a dead reference and raised ``AttributeError: 'NoneType' object has no attribute
'data_ptr'``.  The rebuild and ``refresh`` now take strong references first and drop what is gone themselves."""
import weakref

import torch


def _entry(w):
    cout, cin, kh, kw = w.shape
    return {'ref': weakref.ref(w), 'ptr': w.data_ptr(), 'version': w._version,
            'wb': torch.empty(cout, cin, kh, kw, dtype=torch.bfloat16), 'wt': torch.empty(cin, cout, kh, kw, dtype=torch.bfloat16)}


def _table(weights):
    from stp3_amd import ops
    tab = ops._WeightShadows('cpu')
    for w in weights:
        ent = _entry(w)
        tab.entries[id(w)] = ent
        tab.order.append(ent)
    return tab


def test_rebuild_drops_entries_whose_parameter_died_after_the_callers_check():
    weights = [torch.nn.Parameter(torch.randn(8, 8, 1, 1)) for _ in range(3)]
    tab = _table(weights)
    tab._build_table()
    assert tab.rows == 3
    dead = tab.order[1]
    del weights[1]                                                  # (what a collection inside the rebuild does)
    assert dead['ref']() is None
    tab._build_table()                                              # no liveness check by the caller: the rebuild's own
    assert tab.rows == 2 and dead not in tab.order and len(tab.entries) == 2
    assert all(e['ref']() is w for e, w in zip(tab.order, weights))
    assert sorted(tab.entries) == sorted(id(w) for w in weights)


def test_hold_keeps_the_parameters_alive_for_the_walk():
    weights = [torch.nn.Parameter(torch.randn(8, 8, 1, 1)) for _ in range(2)]
    tab = _table(weights)
    held = tab._hold()
    refs = [e['ref'] for e in tab.order]
    del weights
    assert all(r() is not None for r in refs)                       # the walk can read every parameter
    del held
    assert all(r() is None for r in refs)
    assert tab._hold() == [] and tab.order == [] and tab.entries == {}
