"""Stub steps for the window protocol of run/score_step.StepWindow (host tests, in the manner of tests/md_stubs.py): a "device" whose
replayed step files a loss, raises the overflow counter on planted steps and applies its update only while the counter is zero (the
veto), and whose eager step always applies.  ``applied`` is the log of what moved the weights: ("replay" | "redo", step, batch)."""


def captured_loss(batch, s):
    return 100.0 + 10.0 * batch + s          # what the capped (possibly truncated) step files


def eager_loss(batch, s):
    return 0.5 + 10.0 * batch + s            # what the eager step returns


class StubSteps:
    def __init__(self, ring_len, bad=()):
        self.bad = set(bad)                  # step numbers whose capped list does not fit
        self.step, self.over, self.first_bad = 0, 0, -1
        self.ring = [0.0] * ring_len
        self.applied, self.reads, self.clears = [], 0, 0

    def replay(self, batch):
        s = self.step
        if s in self.bad:
            self.over += 1                   # the builder's counter
        self.ring[s % len(self.ring)] = captured_loss(batch, s)
        if self.over and self.first_bad < 0:
            self.first_bad = s
        if not self.over:                    # the veto
            self.applied.append(("replay", s, batch))
        self.step += 1                       # (the device step cell is never rewound)

    def read(self):
        self.reads += 1
        return self.over, self.first_bad, list(self.ring)

    def clear(self):
        self.clears += 1
        self.over, self.first_bad = 0, -1

    def redo(self, batch, s):
        assert self.over == 0 and self.first_bad == -1, "an eager step must not find the veto standing"
        self.applied.append(("redo", s, batch))
        return eager_loss(batch, s)
