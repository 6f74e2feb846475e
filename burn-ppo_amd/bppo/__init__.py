"""bppo — MI355X-native rollout -> GAE -> PPO-update hot path of burn-ppo.

Host mirror of the reference's surfaces over libbppo.so (include/bppo.h)."""
from ._lib import BppoError, lib  # noqa: F401
from .eval import (EvalStats, TempSchedule, evaluate, evaluate_checkpoints, evaluate_episodes,  # noqa: F401
                   evaluate_pods, generate_permutations, rewards_to_placements)
from .tournament import find_anchor_index, rate_round, round_robin_pods, run_round, swiss_points  # noqa: F401
from .host import make_config, minibatch_sizes, orthogonal_init, schedule_get  # noqa: F401
from .ppo import (ActorCritic, Context, RolloutBuffer, Trainer, VecEnv, collect_rollouts,  # noqa: F401
                  compute_gae, perf_scalars, ppo_update, rollout_episodes, train_step)
from .pool import OpponentPool, OpponentStats, PoolTrainer, RatingHistory  # noqa: F401
from .ratings import (PlackettLuceConfig, PlayerRating, RatingResult, RatingStats, RatingTable,  # noqa: F401
                      compute_ratings)
from .rng import StdRng  # noqa: F401
