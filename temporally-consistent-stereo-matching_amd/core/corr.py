"""Drop-in for the reference's core/corr.py: `CorrBlock1D` on the HIP library.

The class lives in `tcs_mi355.corr` (so the reference's own training script can import it next to its
own `core` package); this module re-exports it for the model (core/tc_stereo.py).
"""
from tcs_mi355.corr import CorrBlock1D  # noqa: F401
