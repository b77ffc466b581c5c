"""Overlay of the reference's `inversion.criteria` package: `inversion.criteria.id_loss` is the MI355X identity loss of training/id_loss.py,
so the reference's unchanged apps (`from inversion.criteria import id_loss as IDLoss`, apps/train_hybrid_encoder.py,
apps/infer_hybrid_encoder.py) get the HIP path; everything else (`inversion.criteria.l2_loss`, `.lpips`, ...) resolves to the reference's
files further down sys.path."""

import pkgutil as _pkgutil
__path__ = _pkgutil.extend_path(__path__, __name__)
