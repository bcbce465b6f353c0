from distributed_reinforcement_learning_amd.algorithms import (
    a2c, vtrace, dqn, burn_in, nstep,
)

__all__ = ["a2c", "vtrace", "dqn", "burn_in", "nstep"]
