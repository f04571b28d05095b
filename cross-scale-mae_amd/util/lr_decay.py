"""Layer-wise learning-rate decay for the ViT (reference util/lr_decay.py, after BEiT / ELECTRA): parameters are grouped by depth and by
whether they are weight-decayed; group `layer_<id>_<decay|no_decay>` carries `lr_scale = layer_decay ** (num_layers - id)`, which
`util.lr_sched.adjust_learning_rate` multiplies into the scheduled rate.  Groups appear in the order their first parameter does in
`model.named_parameters()`; with every depth populated that is 2 * (depth + 2) groups."""


def get_layer_id_for_vit(name, num_layers):
    """Depth of a parameter: 0 for the stem (cls_token, pos_embed, patch_embed.*), i + 1 for blocks.<i>.*, num_layers for what follows the
    last block (final norm, head)."""
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks"):
        return int(name.split(".")[1]) + 1
    return num_layers


def _named_groups(model, weight_decay, no_weight_decay_list, layer_decay, num_layers):
    """{group name: group} in the order the groups first appear — the one grouping rule, behind both functions below."""
    if num_layers is None:
        num_layers = len(model.blocks) + 1
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        decayed = not (p.ndim == 1 or name in no_weight_decay_list)
        layer = get_layer_id_for_vit(name, num_layers)
        key = "layer_%d_%s" % (layer, "decay" if decayed else "no_decay")
        if key not in groups:
            groups[key] = {"lr_scale": layer_decay ** (num_layers - layer), "weight_decay": weight_decay if decayed else 0.0, "params": []}
        groups[key]["params"].append(p)
    return groups


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=(), layer_decay=0.75, num_layers=None):
    """-> [{"lr_scale", "weight_decay", "params"}]: 1-D parameters and the names in `no_weight_decay_list` are not decayed."""
    return list(_named_groups(model, weight_decay, no_weight_decay_list, layer_decay, num_layers).values())


def param_group_names_lrd(model, weight_decay=0.05, no_weight_decay_list=(), layer_decay=0.75, num_layers=None):
    """The group names of param_groups_lrd, in its order (for logs and tests)."""
    return list(_named_groups(model, weight_decay, no_weight_decay_list, layer_decay, num_layers))
