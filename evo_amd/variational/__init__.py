from .eas import (cross, cross_randflip, cross_sparseflip, evolve_states, fitparents, randflip,  # noqa: F401
                  randparents, sparseflip)
from .utils import (init_states, init_states_counter, posterior_scores_host, seed_states_host,  # noqa: F401
                    seed_states_beam_host, swap_states_host, sweep_states_host, vary_Kn)
from .utils import check_remap_index, latent_usage_host, prune_index, remap_states_host  # noqa: F401
from .utils import check_resize, resize_states_host  # noqa: F401
from .eas_counter import evolve_randflip_counter, evolve_states_counter  # noqa: F401
from .utils import neighbour_bound_host  # noqa: F401
