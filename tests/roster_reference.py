"""numpy float64 restatement of the race roster kernels (include/adrp.h adrp_race_roster_*), the yardstick of
tests/test_roster_abi.py (pinned there by a case computed by hand) and of the GPU tests.  Written from the header's
semantics, from hardcoded.HardCodedCommander.predict (the scripted drone's phases) and on tests/agents_reference.py
(the learner columns' bookkeeping, pinned in tests/test_agents_abi.py), one slot at a time."""
import numpy as np

NONE, HARDCODED, POLICY, LEARNER = 0, 1, 2, 3                             # ADRP_ROSTER_*
CMD_NONE, CMD_FULLSTATE, CMD_TAKEOFF, CMD_LAND, CMD_NOTIFY = 0, 1, 2, 5, 10   # ADRP_CMD_*
CMD_ARGS, TIME_SLOT = 14, 13
HARD_FREQ = 25.0            # the scripted controller's own clock (hardcoded.CTRL_FREQ)


def learners_of(roles):
    """the learner drones in roster order: learner l is drone learners_of(roles)[l]"""
    return [n for n, r in enumerate(roles) if r == LEARNER]


class Roster:
    """clock int32 [E], phase uint8 [3, E N]; ref float64 [E, N, L, 3], offset int64 [E, N] for the scripted drones"""

    def __init__(self, E, N, roles, ctrl_freq, ref=None, offset=None):
        self.E, self.N, self.roles, self.ctrl_freq = int(E), int(N), list(roles), float(ctrl_freq)
        assert len(self.roles) == self.N
        self.learners = learners_of(self.roles)
        self.ref = None if ref is None else np.asarray(ref, np.float64)
        self.offset = None if offset is None else np.asarray(offset, np.int64).reshape(self.E, self.N)
        self.clock = np.zeros(self.E, np.int32)
        self.phase = np.zeros((3, self.E * self.N), np.uint8)

    def act(self, setpoints=None, learner_act=None):
        """-> codes int32 [E, N], args float64 [E, N, 14]; setpoints float32 [N, E, 4], learner_act float32 [L, E, 4]"""
        E, N = self.E, self.N
        codes = np.zeros((E, N), np.int32)
        args = np.zeros((E, N, CMD_ARGS), np.float64)
        for e in range(E):
            ep_time = np.float64(self.clock[e]) / np.float64(self.ctrl_freq)
            for n in range(N):
                role, slot, a = self.roles[n], e * N + n, args[e, n]
                if role == HARDCODED:
                    L = self.ref.shape[2]
                    step = min(max(int(np.trunc(ep_time * HARD_FREQ)) - int(self.offset[e, n]), 0), L)
                    took, notified, landed = (bool(x) for x in self.phase[:, slot])
                    if not took:
                        codes[e, n], a[0], a[1], a[TIME_SLOT] = CMD_TAKEOFF, 0.3, 2.0, 2.0
                        self.phase[0, slot] = 1
                    elif step < L:
                        codes[e, n] = CMD_FULLSTATE
                        a[0:3], a[6:9], a[TIME_SLOT] = self.ref[e, n, step], 0.5, ep_time
                    elif not notified:
                        codes[e, n], a[0], a[TIME_SLOT] = CMD_NOTIFY, ep_time, ep_time
                        self.phase[1, slot] = 1
                    elif not landed:
                        codes[e, n], a[1], a[TIME_SLOT] = CMD_LAND, 2.0, 2.0
                        self.phase[2, slot] = 1
                elif role in (POLICY, LEARNER):
                    s = setpoints[n, e] if role == POLICY else learner_act[self.learners.index(n), e]
                    s = np.asarray(s, np.float32).astype(np.float64)
                    codes[e, n] = CMD_FULLSTATE
                    a[0:3], a[9], a[TIME_SLOT] = s[0:3], s[3], ep_time
        return codes, args

    def tick(self, mask=None):
        for e in range(self.E):
            if mask is None or mask[e]:
                self.clock[e] = 0
                self.phase[:, e * self.N:(e + 1) * self.N] = 0
            else:
                self.clock[e] += 1


STATE = ("wr_gate", "wr_target", "wr_prev", "alive", "run_return", "run_length")
OUTPUTS = ("rewards", "valid", "next_start", "ep_return", "ep_length", "raw", "stored", "boot")


def compact_step(ag, learners, obs, gate, flags, term, trunc, boot_value, gamma):
    """adrp_race_roster_step on ``ag`` (an agents_reference.Agents of all E N slots): the learner drones' slots take
    Agents.step with boot_value [L E] read at column l E + e; the outputs of slot e N + learners[l] go to that
    column; the state of every other slot stays as it is -> Agents.step's dict, each [L E]"""
    E, N, L = ag.E, ag.N, len(learners)
    slot = np.array([[e * N + n for e in range(E)] for n in learners]).reshape(L * E)     # column -> slot
    full_boot = np.full(E * N, np.nan, np.float32)
    full_boot[slot] = np.asarray(boot_value, np.float32).reshape(L * E)
    others = np.setdiff1d(np.arange(E * N), slot)
    keep = {k: getattr(ag, k)[others].copy() for k in STATE}
    # a slot that is not a learner's is stepped as a dead one (nothing of its row is read) and then put back
    alive = ag.alive.copy()
    ag.alive[others] = 0
    out = ag.step(obs, gate, flags, term, trunc, full_boot, gamma)
    ag.alive[others] = alive[others]
    for k in STATE:
        assert np.array_equal(getattr(ag, k)[others], keep[k], equal_nan=True)
    return {k: out[k][slot] for k in OUTPUTS}
