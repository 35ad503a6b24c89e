#!/usr/bin/env python
"""Records tests/golden/lrd_groups_vit_small.json: the layer-wise parameter groups the REFERENCE builds (``param_groups_lrd`` of its
``models/lr_decay.py``) for this package's ``vit_small``, as parameter names and numbers.  tests/test_optim_recipe.py holds
``mvsformer_amd.optim.vit_param_groups`` against it.

    python tools/gen_optim_golden.py /path/to/reference/checkout
"""
import importlib.util
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VIT_LR, WEIGHT_DECAY, LAYER_DECAY = 3e-5, 0.05, 0.75
NO_DECAY = ["pos_embed", "cls_token"]


def main(checkout):
    spec = importlib.util.spec_from_file_location("reference_lr_decay", os.path.join(checkout, "models", "lr_decay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from mvsformer_amd.vit import vit_small
    vit = vit_small()
    names = {id(p): n for n, p in vit.named_parameters()}
    groups = mod.param_groups_lrd(vit, VIT_LR, weight_decay=WEIGHT_DECAY, no_weight_decay_list=NO_DECAY, layer_decay=LAYER_DECAY)
    out = {"vit_lr": VIT_LR, "weight_decay": WEIGHT_DECAY, "layer_decay": LAYER_DECAY, "no_weight_decay_list": NO_DECAY,
           "groups": [{"params": [names[id(p)] for p in g["params"]], "lr": g["lr"], "lr_scale": g["lr_scale"], "weight_decay": g["weight_decay"],
                       "vit_param": g["vit_param"]} for g in groups]}
    path = os.path.join(REPO, "tests", "golden", "lrd_groups_vit_small.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%s: %d groups, %d tensors" % (path, len(out["groups"]), sum(len(g["params"]) for g in out["groups"])))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
