"""Host-side checks of per-group learning rates on the parameter arena (no GPU): the grouped entry point is declared, bound and exported;
the arena's run table from torch-style groups; the 1x / 10x partition of every network with a pretrainable encoder; the multi-group
state dict form; the command line's tape decision for --diff-lr."""
import pathlib
import re

import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_grouped_entry_point_is_declared_bound_and_exported():
    import __graft_entry__
    __graft_entry__.build(only_library=True)
    from supervised_dispnet_amd import _lib
    lib = _lib.load()
    header = (ROOT / "include" / "dispnet_hip.h").read_text()
    m = re.search(r"\bint\s+dn_sgd_step_groups\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, "dn_sgd_step_groups is not declared in include/dispnet_hip.h"
    declared = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    assert len(declared) == 14 and len(_lib.SIGNATURES["dn_sgd_step_groups"][1]) == 14
    assert hasattr(lib, "dn_sgd_step_groups")
    assert lib.dn_version() == _lib.EXPECTED_ABI >= 23
    assert "`dn_sgd_step_groups`" in (ROOT / "INTEGRATION.md").read_text()


SHAPES = [(4, 3, 3, 3), (5,), (17,), (6, 4), (1, 2, 3, 3), (8,)]       # 108, 5 (+3), 17 (+3), 24, 18 (+2), 8 elements


def _params(seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def test_run_table_of_interleaved_groups_with_padded_slices():
    from supervised_dispnet_amd.optim import ParamArena
    ps = _params()
    before = [p.detach().clone() for p in ps]
    groups = [{"params": [ps[0], ps[2], ps[5]], "lr": 1e-2}, {"params": [ps[1], ps[3], ps[4]], "lr": 1e-1}]
    order = [ps[i] for i in (3, 0, 2, 4, 1, 5)]                       # groups 1 0 0 1 1 0 in production order
    arena = ParamArena(groups, production_order=order)
    assert [id(p) for p in arena.params] == [id(p) for p in order]    # the slice order stays the production order
    assert arena.offsets == [0, 24, 132, 152, 172, 180] and arena.numel == 188
    assert arena.n_groups == 2 and arena.group_of == [1, 0, 0, 1, 1, 0]
    # runs of equal group; the 17-element slice's padding (149..151) is inside group 0's run, the 18- and 5-element ones' in group 1's
    assert arena.runs == [(24, 1), (152, 0), (180, 1), (188, 0)]
    assert all(e % 4 == 0 for e, _ in arena.runs)
    assert [id(p) for p in arena.listed] == [id(p) for p in (ps[0], ps[2], ps[5], ps[1], ps[3], ps[4])]     # torch's index order
    assert arena.listed_group == [0, 0, 0, 1, 1, 1]
    assert arena.group_options == [{"lr": 1e-2}, {"lr": 1e-1}]
    for p, b in zip(ps, before):                                      # the parameters now live in the arena, values kept
        assert torch.equal(p.detach(), b)
        assert arena.flat_p.data_ptr() <= p.data_ptr() < arena.flat_p.data_ptr() + 4 * arena.numel


def test_run_table_alternating_on_every_slice_and_without_production_order():
    from supervised_dispnet_amd.optim import ParamArena, group_runs
    ps = _params()
    arena = ParamArena([{"params": ps[0::2], "lr": 1.0}, {"params": ps[1::2], "lr": 2.0}], production_order=ps)
    assert arena.group_of == [0, 1, 0, 1, 0, 1]
    assert arena.runs == [(108, 0), (116, 1), (136, 0), (160, 1), (180, 0), (188, 1)]
    ps = _params()
    arena = ParamArena([{"params": ps[:2]}, {"params": ps[2:]}])      # no production order: construction order
    assert arena.runs == [(116, 0), (188, 1)]
    assert group_runs([0, 4, 8], 12, [2, 2, 2]) == [(12, 2)]


def test_one_group_is_the_flat_arena():
    from supervised_dispnet_amd.optim import ParamArena
    order = (3, 0, 4, 2, 1, 5)
    ps_a, ps_b, ps_c = _params(), _params(), _params()
    flat = ParamArena(ps_a, production_order=[ps_a[i] for i in order])
    one = ParamArena([{"params": ps_b, "lr": 0.5}], production_order=[ps_b[i] for i in order])
    bare = ParamArena([{"params": ps_c}], production_order=[ps_c[i] for i in order])
    for a in (flat, one, bare):
        assert a.n_groups == 1 and a.runs == [(a.numel, 0)] and a.group_of == [0] * 6
        assert a.offsets == flat.offsets and torch.equal(a.flat_p, flat.flat_p)
    assert flat.group_options == [{}] and one.group_options == [{"lr": 0.5}]


def test_groups_that_overlap_or_miss_a_trainable_parameter_are_refused():
    from supervised_dispnet_amd.optim import ParamArena, split_param_groups
    ps = _params()
    with pytest.raises(ValueError, match="more than one parameter group"):
        ParamArena([{"params": ps[:3]}, {"params": ps[2:]}], production_order=ps)
    with pytest.raises(ValueError, match="more than one parameter group"):
        split_param_groups([{"params": [ps[0], ps[0]]}, {"params": ps[1:]}])
    with pytest.raises(ValueError, match="miss 1 trainable parameter"):
        ParamArena([{"params": ps[:3]}, {"params": ps[4:]}], production_order=ps)
    with pytest.raises(ValueError, match="not a dict with a 'params' entry"):
        split_param_groups([{"params": ps[:3]}, ps[3:]])
    # a frozen parameter of the production order is nobody's to list
    ps[3].requires_grad_(False)
    arena = ParamArena([{"params": ps[:3]}, {"params": ps[4:]}], production_order=ps)
    assert len(arena.params) == 5 and arena.runs == [(136, 0), (164, 1)]
    # nothing was re-pointed by the refused constructions
    fresh = _params()
    where = [p.data_ptr() for p in fresh]
    with pytest.raises(ValueError):
        ParamArena([{"params": fresh[:3]}, {"params": fresh[4:]}], production_order=fresh)
    assert [p.data_ptr() for p in fresh] == where and not any(hasattr(p, "_dn_grad_view") for p in fresh)


def test_a_differing_key_besides_lr_is_refused():
    from supervised_dispnet_amd.optim import FusedAdam, FusedSGD, ParamArena, split_param_groups
    ps = _params()
    where = [p.data_ptr() for p in ps]
    with pytest.raises(ValueError, match="weight_decay.*only lr may differ"):
        ParamArena([{"params": ps[:3], "lr": 1.0, "weight_decay": 0.0}, {"params": ps[3:], "lr": 2.0, "weight_decay": 5e-4}])
    with pytest.raises(ValueError, match="momentum.*only lr may differ"):
        split_param_groups([{"params": ps[:3], "momentum": 0.9}, {"params": ps[3:], "momentum": 0.8}])
    # the same value in every group that sets it is no difference ...
    listed, group_of, options = split_param_groups([{"params": ps[:3], "lr": 1.0, "momentum": 0.9}, {"params": ps[3:], "lr": 2.0}])
    assert len(listed) == 6 and group_of == [0, 0, 0, 1, 1, 1] and options == [{"lr": 1.0, "momentum": 0.9}, {"lr": 2.0}]
    # ... but the optimizer holds it against its own value, and knows no other option; both before anything is moved or needs a device
    with pytest.raises(ValueError, match="group 0 sets momentum=0.9, the optimizer has 0.5"):
        FusedSGD([{"params": ps[:3], "lr": 1.0, "momentum": 0.9}, {"params": ps[3:], "lr": 2.0}], momentum=0.5)
    with pytest.raises(ValueError, match="group 1 sets betas="):
        FusedSGD([{"params": ps[:3], "lr": 1.0}, {"params": ps[3:], "lr": 2.0, "betas": (0.9, 0.99)}], momentum=0.9)
    with pytest.raises(ValueError, match="no learning rate for parameter group 1"):
        FusedSGD([{"params": ps[:3], "lr": 1.0}, {"params": ps[3:]}], momentum=0.9)
    with pytest.raises(ValueError, match="FusedAdam takes one parameter group"):
        FusedAdam([{"params": ps[:3], "lr": 1.0}, {"params": ps[3:], "lr": 2.0}])
    assert [p.data_ptr() for p in ps] == where and not any(hasattr(p, "_dn_grad_view") for p in ps)


NETWORKS = ["Disp_vgg_BN", "Disp_vgg_BN_DORN", "Disp_vgg", "Disp_vgg_feature", "Disp_res_50", "Disp_res_18", "Disp_res", "Disp_res_101",
            "FCRN", "deeplab_depth", "res50_aspp", "monodepth2"]
ENCODER_PREFIXES = {"Disp_vgg_BN": ("features.features.",), "Disp_vgg_BN_DORN": ("features.features.",),
                    "Disp_vgg": ("conv1.", "conv2.", "conv3.", "conv4.", "conv5."), "Disp_vgg_feature": ("features.features.",),
                    "deeplab_depth": ("Scale.conv1.", "Scale.bn1.", "Scale.layer1.", "Scale.layer2.", "Scale.layer3.", "Scale.layer4."),
                    "monodepth2": ("encoder.",)}
ENCODER_PREFIXES["res50_aspp"] = ENCODER_PREFIXES["deeplab_depth"]
RESNET_PREFIXES = ("conv1.", "bn1.", "layer1.", "layer2.", "layer3.", "layer4.")


def _build(name):
    import supervised_dispnet_amd.models as models
    if name == "monodepth2":
        import supervised_dispnet_amd.networks as networks
        enc = networks.ResnetEncoder(num_layers=18, pretrained=False)
        return models.monodepth2(encoder=enc, decoder=networks.DepthDecoder(enc.num_ch_enc))
    if name == "Disp_vgg":
        return models.Disp_vgg()
    if name == "Disp_vgg_BN_DORN":
        return models.Disp_vgg_BN_DORN(ordinal_c=16, datasets="kitti")
    return getattr(models, name)(datasets="kitti")


@pytest.mark.parametrize("name", NETWORKS)
def test_the_two_groups_partition_the_trainable_hot_parameters(name):
    net = _build(name)
    names = {id(p): n for n, p in net.named_parameters()}
    one, ten = list(net.get_1x_lr_params()), list(net.get_10x_lr_params())
    assert not isinstance(net.get_1x_lr_params(), list)                # generators, as in the reference
    hot = [p for p in net._hot_parameters() if p.requires_grad]
    assert one and ten
    assert len({id(p) for p in one}) == len(one) and len({id(p) for p in ten}) == len(ten)
    assert not {id(p) for p in one} & {id(p) for p in ten}
    assert {id(p) for p in one} | {id(p) for p in ten} == {id(p) for p in hot} and len(one) + len(ten) == len(hot)
    assert all(p.requires_grad for p in one + ten)
    prefixes = ENCODER_PREFIXES.get(name, RESNET_PREFIXES)
    assert all(names[id(p)].startswith(prefixes) for p in one), [names[id(p)] for p in one if not names[id(p)].startswith(prefixes)]
    assert not any(names[id(p)].startswith(prefixes) for p in ten)
    assert not any(".classifier." in names[id(p)] for p in one + ten)
    # 10x is the decoder and the heads: every name there says so
    decoder = ("upconv", "iconv", "disp", "predict_disp", "up1.", "up2.", "up3.", "up4.", "conv2.", "bn2.", "conv3.", "Scale.layer5.",
               "conv_ord.", "decoder.")
    assert all(names[id(p)].startswith(decoder) for p in ten), [names[id(p)] for p in ten if not names[id(p)].startswith(decoder)]
    # and the arena takes the two groups with the network's production order (nothing missed, nothing twice)
    if hasattr(net, "_grad_production_order"):
        from supervised_dispnet_amd.optim import group_runs
        order = [p for p in net._grad_production_order() if p.requires_grad]
        assert {id(p) for p in order} == {id(p) for p in hot}
        in_one = {id(p) for p in one}
        runs = group_runs(list(range(0, 4 * len(order), 4)), 4 * len(order), [0 if id(p) in in_one else 1 for p in order])
        assert len(runs) == 2 and runs[0][1] == 1 and runs[1][1] == 0   # backward writes the decoder first, then the encoder


def test_frozen_parameters_are_in_neither_group():
    import supervised_dispnet_amd.models as models
    net = models.Disp_vgg_BN(datasets="kitti", with_classifier=False)
    conv0 = net.features.features[0]
    conv0.weight.requires_grad_(False)
    one = list(net.get_1x_lr_params())
    assert all(p is not conv0.weight for p in one) and any(p is conv0.bias for p in one)
    assert len(one) + len(list(net.get_10x_lr_params())) == len(list(net._hot_parameters())) - 1


def test_networks_without_a_pretrained_encoder_have_no_groups_and_keep_the_exit_text():
    import supervised_dispnet_amd.models as models
    for cls in (models.DispNetS, models.PoseExpNet):
        assert not hasattr(cls, "get_1x_lr_params") and not hasattr(cls, "get_10x_lr_params")
    src = (ROOT / "train.py").read_text()
    assert ('raise SystemExit("--diff-lr needs a network with get_1x_lr_params() / get_10x_lr_params() (reference: models.DORN only)")'
            in src)
    assert "torch.optim.SGD(" not in src and "plain_params" not in src


def test_multi_group_state_dict_form_and_grouping_check():
    from supervised_dispnet_amd.optim import ParamArena, flat_momentum_from_torch_sgd, grouped_state, require_same_grouping
    ps = _params()
    ref_groups = [{"params": [ps[0], ps[2], ps[5]], "lr": 1e-2}, {"params": [ps[1], ps[3], ps[4]], "lr": 1e-1}]
    ref = torch.optim.SGD(ref_groups, lr=1e-2, momentum=0.9, weight_decay=5e-4)
    g = torch.Generator().manual_seed(9)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    sd = ref.state_dict()
    for p in ps:
        p.grad = None
    arena = ParamArena(ref_groups, production_order=[ps[i] for i in (3, 0, 2, 4, 1, 5)])
    hyper = [{"params": grp["params"], "lr": grp["lr"], "momentum": 0.9, "weight_decay": 5e-4, "dampening": 0, "nesterov": False}
             for grp in ref_groups]
    own = grouped_state(hyper, arena.listed_group)
    assert own == [{"lr": 1e-2, "momentum": 0.9, "weight_decay": 5e-4, "dampening": 0, "nesterov": False, "params": [0, 1, 2]},
                   {"lr": 1e-1, "momentum": 0.9, "weight_decay": 5e-4, "dampening": 0, "nesterov": False, "params": [3, 4, 5]}]
    assert [grp["params"] for grp in own] == [grp["params"] for grp in sd["param_groups"]]            # torch's own indices
    # round trip: the own form and torch's pass the grouping check of an optimizer with groups of 3 + 3 ...
    require_same_grouping({"param_groups": own}, [3, 3])
    require_same_grouping(sd, [3, 3])
    # ... and torch's two-group state lands in the permuted arena's slices
    flat = flat_momentum_from_torch_sgd(sd, arena.listed, arena)
    for p, o in zip(arena.params, arena.offsets):
        assert torch.equal(flat[o:o + p.numel()].view(p.shape), ref.state[p]["momentum_buffer"])
    for bad in ([2, 4], [6], [3, 3, 0], [3]):
        with pytest.raises(ValueError, match=r"groups of sizes \[3, 3\], this optimizer has groups of sizes"):
            require_same_grouping(sd, bad)
    with pytest.raises(ValueError, match=r"sizes \[None\]"):           # a one-group FusedSGD state (no "params") into two groups
        require_same_grouping({"param_groups": [{"lr": 1e-2}]}, [3, 3])
    with pytest.raises(ValueError, match=r"sizes \[\]"):
        require_same_grouping({"momentum_buffer": flat}, [3, 3])


def test_diff_lr_goes_on_the_launch_tape_with_an_arena_optimizer():
    import train
    args = train.build_parser().parse_args(["DATA", "--with-gt", "--loss", "L1", "--diff-lr", "--network", "disp_vgg_BN"])
    assert args.diff_lr and args.tape is None                          # no flag: the tape is the default where the setting is eligible

    class Fused(object):
        arena = object()

    assert train.tape_refusal(args, Fused()) is None
    args.loss = "DORN"
    assert train.tape_refusal(args, Fused()) == "only the supervised depth losses are taped"


def test_diff_lr_groups_are_the_networks_two_at_lr_and_ten_times_lr():
    import supervised_dispnet_amd.models as models
    import train
    net = models.Disp_res_18(datasets="kitti")
    groups = train.diff_lr_groups(net, 1e-3)
    assert [g["lr"] for g in groups] == [1e-3, 1e-2]
    assert [id(p) for p in groups[0]["params"]] == [id(p) for p in net.get_1x_lr_params()]
    assert [id(p) for p in groups[1]["params"]] == [id(p) for p in net.get_10x_lr_params()]
