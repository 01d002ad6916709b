from ._models import Model  # noqa: F401
from .bsc import BSC  # noqa: F401
from .sssc import SSSC  # noqa: F401
from .generate import generate_counter  # noqa: F401
from .exact import enumerate_chunk, fold_exact  # noqa: F401
from .predictive import predictive_moments_host  # noqa: F401
from .predictive_score import pit_summary, predictive_log_score_host  # noqa: F401
from .posterior_sample import sample_posterior_counter  # noqa: F401
from .loglik_estimate import estimate_log_likelihood_counter, proposal_of  # noqa: F401
from .remap import remap_theta  # noqa: F401
from .ais import ais_conditional, ais_log_likelihood_counter, ais_posterior_counter, ais_scalars, sigmoid_schedule  # noqa: F401
from .ais import ais_admit_candidates_host, state_digest  # noqa: F401
