"""bppo — MI355X-native rollout -> GAE -> PPO-update hot path of burn-ppo.

Host mirror of the reference's surfaces over libbppo.so (include/bppo.h)."""
from ._lib import BppoError, lib  # noqa: F401
from .eval import (EvalStats, TempSchedule, evaluate, evaluate_checkpoints, evaluate_episodes,  # noqa: F401
                   evaluate_pods, generate_permutations, rewards_to_placements)
from .tournament import (Contestant, DeviceEngine, TournamentResult, assign_byes, find_anchor_index,  # noqa: F401
                         form_dutch_pods, form_dutch_pods_with_floaters, has_repeat_opponents, pod_avg_points,
                         pod_full_draws, pod_summary, rate_round, round_pods, round_robin_pods, run_round,
                         run_tournament, split_round, swiss_pods, swiss_points, tournament_format,
                         update_stats_from_games)
from .host import make_config, minibatch_sizes, orthogonal_init, schedule_get  # noqa: F401
from .ppo import (ActorCritic, Context, RolloutBuffer, Trainer, VecEnv, collect_rollouts,  # noqa: F401
                  compute_gae, perf_scalars, ppo_update, rollout_episodes, train_step)
from .episodes import (EpisodeWindow, debug_episode_stats, episode_stats, rollout_episode_outcomes,  # noqa: F401
                       set_episode_stats)
from .pool import OpponentPool, OpponentStats, PoolTrainer, RatingHistory  # noqa: F401
from .ratings import (PlackettLuceConfig, PlayerRating, RatingResult, RatingStats, RatingTable,  # noqa: F401
                      compute_ratings)
from .rng import StdRng  # noqa: F401
