"""The fused autograd nodes address their forward arguments by name (HF._Slots): the declared table of each node is the signature of its
forward, backward's tuple has one slot per argument, and a gradient filed under a name that is no argument raises (CPU)."""
import inspect

import pytest

NODES = ["BlockFn", "TailBlockFn", "AttentionFn", "MlpFn"]


@pytest.mark.parametrize("node", NODES)
def test_declared_names_are_the_forward_signature(node):
    from UCF_VIT._hip import functional as HF
    fn = getattr(HF, node)
    params = list(inspect.signature(fn.forward).parameters)
    assert params[0] == "ctx"
    assert fn.ARGS.names == tuple(params[1:])
    assert len(set(fn.ARGS.names)) == len(fn.ARGS.names)


@pytest.mark.parametrize("node", NODES)
def test_gradients_are_filed_by_name(node):
    from UCF_VIT._hip import functional as HF
    args = getattr(HF, node).ARGS
    n = len(args.names)
    assert args.grads() == (None,) * n
    for i, name in enumerate(args.names):                              # every name fills its own slot and no other
        out = args.grads(**{name: i + 1})
        assert len(out) == n and out[i] == i + 1 and all(g is None for j, g in enumerate(out) if j != i)
    with pytest.raises(KeyError):
        args.grads(not_an_argument=1)

    class Ctx:
        needs_input_grad = tuple(i % 2 == 0 for i in range(n))
    need = args.needs(Ctx)
    assert list(need) == list(args.names) and [need[k] for k in args.names] == list(Ctx.needs_input_grad)

    class Short:                                                       # apply() with the defaulted arguments left out
        needs_input_grad = (True,) * 3
    need = args.needs(Short)
    assert list(need) == list(args.names) and [need[k] for k in args.names] == [True] * 3 + [False] * (n - 3)


def test_tail_node_differs_from_the_dense_one_by_the_group_handle_alone():
    from UCF_VIT._hip import functional as HF
    assert [n for n in HF.BlockFn.ARGS.names if n != "tp"] == list(HF.TailBlockFn.ARGS.names)
