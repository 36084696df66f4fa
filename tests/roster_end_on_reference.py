"""numpy restatement of ``adrp_race_roster_done`` (include/adrp_train.h, csrc/roster_kernel.h): the reset mask of a
roster collector that ends an env with its last learner.  CPU only."""
import numpy as np


def done_mask(alive, term, trunc, num_drones, learners):
    """alive uint8 [E N] as the learners' step left it, term / trunc [E], learners: the learner drones' indices
    -> uint8 [E]: 1 where the race is over (term | trunc) or no learner drone of the env is alive, else 0.  The
    alive of the other slots is not read."""
    term, trunc = np.asarray(term).astype(bool), np.asarray(trunc).astype(bool)
    E = term.shape[0]
    alive = np.asarray(alive).reshape(E, num_drones)
    out = np.zeros(E, np.uint8)
    for e in range(E):
        any_alive = any(alive[e, n] != 0 for n in learners)
        out[e] = 1 if (term[e] or trunc[e] or not any_alive) else 0
    return out
