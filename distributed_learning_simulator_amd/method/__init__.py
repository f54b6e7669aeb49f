"""Importing this package registers every method (reference `method/__init__.py:1-9`).
`fed_gcn` and `fed_aas` have no package of their own: `fed_gnn` registers them."""

from . import fed_avg  # noqa: F401  isort: skip
from . import (fed_dropout_avg, fed_paq, fed_obd, shapley_value, sign_sgd, smafd, fed_gnn, fed_topk,  # noqa: F401  isort: skip
               fed_trimmed_mean, fed_median, fed_krum, fed_multi_krum, fed_prox, fed_scaffold, fed_dp_avg, fed_avgm,
               fed_adagrad, fed_adam, fed_yogi, fed_secagg, fed_drive)
from .algorithm_factory import CentralizedAlgorithmFactory

__all__ = ["CentralizedAlgorithmFactory"]
