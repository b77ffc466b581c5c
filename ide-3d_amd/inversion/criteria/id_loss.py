"""`inversion.criteria.id_loss` for the reference's unchanged apps: `IDLoss()` is `training.id_loss.IDLoss` with the reference's
constructor, which loads the IR-SE50 weights from `inversion.configs.paths_config.ir_se50` (inversion/criteria/id_loss.py:9-16)."""

import inversion.configs.paths_config as path_config
from training import id_loss as _id_loss
from training.id_loss import Backbone  # noqa: F401


class IDLoss(_id_loss.IDLoss):
    def __init__(self):
        print('Loading ResNet ArcFace')
        super().__init__(weights=path_config.ir_se50)
