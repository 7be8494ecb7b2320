"""Host-side checks of the fused SGD path (no GPU): the two C entry points are declared, bound and exported; a torch.optim.SGD state
dict converts into the arena's flat momentum buffer; the command line round-trips; the launch tape's refusal text."""
import pathlib
import re

import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_sgd_entry_points_are_declared_bound_and_exported():
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    from supervised_dispnet_amd import _lib
    lib = _lib.load()
    header = (ROOT / "include" / "dispnet_hip.h").read_text()
    for name in ("dn_sgd_step", "dn_sgd_step_dev"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, "%s is not declared in include/dispnet_hip.h" % name
        declared = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        assert name in _lib.SIGNATURES, "ctypes binding missing for %s" % name
        assert len(_lib.SIGNATURES[name][1]) == len(declared), (name, len(_lib.SIGNATURES[name][1]), len(declared))
        assert hasattr(lib, name), "libdispnet_hip.so does not export %s" % name
    assert len(_lib.SIGNATURES["dn_sgd_step"][1]) == 9 and len(_lib.SIGNATURES["dn_sgd_step_dev"][1]) == 8


SHAPES = [(4, 3, 3, 3), (5,), (17,), (6, 4), (1, 2, 3, 3)]


def _arena_and_torch_state(skip=None, momentum=0.9):
    """Five CPU parameters, an arena that orders them by a permuted production order, and the state dict of a torch.optim.SGD over
    the parameter list after two steps (`skip`: index of a parameter that never gets a gradient)."""
    from supervised_dispnet_amd.optim import ParamArena
    g = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]
    ref = torch.optim.SGD(params, lr=1e-2, momentum=momentum, weight_decay=5e-4)
    for it in range(2):
        for i, p in enumerate(params):
            p.grad = None if i == skip else torch.randn(p.shape, generator=g)
        ref.step()
    sd = ref.state_dict()
    for p in params:
        p.grad = None
    order = [params[i] for i in (3, 0, 4, 2, 1)]
    arena = ParamArena(params, production_order=order)
    assert [id(p) for p in arena.params] == [id(p) for p in order]
    return params, arena, sd, ref


def test_torch_sgd_state_lands_in_the_permuted_arena_slices_and_padding_stays_zero():
    from supervised_dispnet_amd.optim import flat_momentum_from_torch_sgd
    params, arena, sd, ref = _arena_and_torch_state()
    flat = flat_momentum_from_torch_sgd(sd, params, arena)
    assert flat.shape == (arena.numel,) and flat.dtype == torch.float32 and flat.device.type == "cpu"
    covered = torch.zeros(arena.numel, dtype=torch.bool)
    for p, o in zip(arena.params, arena.offsets):
        want = ref.state[p]["momentum_buffer"]
        assert torch.equal(flat[o:o + p.numel()].view(p.shape), want)
        covered[o:o + p.numel()] = True
    assert arena.numel > sum(p.numel() for p in params)             # the 5-, 17- and 18-element slices are padded
    assert int((~covered).sum()) == arena.numel - sum(p.numel() for p in params)
    assert torch.equal(flat[~covered], torch.zeros(int((~covered).sum())))
    assert float(flat[covered].abs().min()) > 0


def test_torch_sgd_state_missing_entry_loads_as_zeros():
    from supervised_dispnet_amd.optim import flat_momentum_from_torch_sgd
    params, arena, sd, ref = _arena_and_torch_state(skip=2)
    assert 2 not in sd["state"] and len(sd["state"]) == 4
    flat = flat_momentum_from_torch_sgd(sd, params, arena)
    for p, o in zip(arena.params, arena.offsets):
        got = flat[o:o + p.numel()]
        if p is params[2]:
            assert torch.equal(got, torch.zeros(17))
        else:
            assert torch.equal(got.view(p.shape), ref.state[p]["momentum_buffer"])


def test_torch_sgd_state_with_wrong_shape_or_count_is_refused():
    from supervised_dispnet_amd.optim import flat_momentum_from_torch_sgd
    params, arena, sd, _ = _arena_and_torch_state()
    bad = {"state": {k: dict(v) for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]}
    bad["state"][3]["momentum_buffer"] = torch.zeros(4, 6)
    with pytest.raises(ValueError, match=r"parameter 3\b"):
        flat_momentum_from_torch_sgd(bad, params, arena)
    with pytest.raises(ValueError, match="5 parameters.*built from 4"):
        flat_momentum_from_torch_sgd(sd, params[:4], arena)
    groups = [dict(sd["param_groups"][0], params=list(range(6)))]
    with pytest.raises(ValueError, match="6 parameters.*built from 5"):
        flat_momentum_from_torch_sgd({"state": sd["state"], "param_groups": groups}, params, arena)
    stray = {"state": dict(sd["state"]), "param_groups": sd["param_groups"]}
    stray["state"][7] = {"momentum_buffer": torch.zeros(5)}
    with pytest.raises(ValueError, match=r"parameter 7\b"):
        flat_momentum_from_torch_sgd(stray, params, arena)


def test_parser_round_trips_the_sgd_flags():
    import train
    args = train.build_parser().parse_args(["DATA", "--sgd", "--momentum", "0.9", "--wd", "5e-4"])
    assert args.sgd is True and args.momentum == 0.9 and args.weight_decay == 5e-4 and not args.diff_lr
    assert train.build_parser().parse_args(["DATA"]).sgd is False


def test_tape_refusal_text_names_diff_lr_only():
    import train
    args = train.build_parser().parse_args(["DATA", "--with-gt", "--loss", "L1", "--sgd"])

    class Fused(object):
        arena = object()

    plain = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    assert train.tape_refusal(args, Fused()) is None
    assert train.tape_refusal(args, plain) == "needs a fused optimizer (not --diff-lr)"
    args.unsupervised = True
    assert train.tape_refusal(args, Fused()) == "only the supervised depth losses are taped"
    assert train.optimizer_state_name(Fused()) == "the SGD momentum buffer starts"
