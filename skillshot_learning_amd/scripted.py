"""Scripted actors — fixed closed-form policies on the game state.

`evaluate`, `league` and `train_vs` seat nets; a ScriptedActor sits wherever
one of those does and gives their numbers an absolute anchor (a league Elo
"above chaser", a first win rate for an untrained net, a training opponent
before any checkpoint exists).  Four kinds (include/skillshot.h SK_BOT_*, the
policy in csrc/sk_bot.hpp):

    still   never moves or turns
    random  the keyed random policy (VecSkillshotGame.gen_random_actions)
    aimer   turns towards the opponent, never moves
    chaser  turns towards the opponent and walks up to 8 player sizes of it

Every seat keeps auto-firing, as a net's does: the step does that.  A scripted
actor acts on the env's STATE, not on observations: `actions(env)` is one
small launch (sk_env_bot_act) on either backend, and the one-launch league and
pool kernels compute the policy themselves for a scripted seat.
"""
from . import _capi

KINDS = {"still": _capi.SK_BOT_STILL, "random": _capi.SK_BOT_RANDOM, "aimer": _capi.SK_BOT_AIMER,
         "chaser": _capi.SK_BOT_CHASER}
NAMES = {code: name for name, code in KINDS.items()}


def kind_code(kind):
    """a kind given by name or by code, as its code"""
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"unknown scripted actor {kind!r}: one of {sorted(KINDS)}")
        return KINDS[kind]
    if isinstance(kind, bool) or not isinstance(kind, int) or kind not in NAMES:
        raise ValueError(f"a scripted actor's kind is one of {sorted(KINDS)} or a code in [1, 4], not {kind!r}")
    return int(kind)


class ScriptedActor:
    """ScriptedActor("chaser") or ScriptedActor(4): `kind` holds the code,
    `name` the name."""

    def __init__(self, kind):
        self.kind = kind_code(kind)
        self.name = NAMES[self.kind]

    def actions(self, env, out=None):
        """both seats' actions [2, N, 2] on env's current state"""
        return env.bot_actions(self.kind, out=out)

    def __repr__(self):
        return f"ScriptedActor({self.name!r})"


def as_scripted(entry):
    """the ScriptedActor an actor entry names (itself, or one of the four
    strings), or None for any other entry (another string included: the
    caller refuses it as it refuses any entry it does not know)"""
    if isinstance(entry, ScriptedActor):
        return entry
    if isinstance(entry, str) and entry in KINDS:
        return ScriptedActor(entry)
    return None
