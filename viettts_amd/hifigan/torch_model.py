"""vietTTS/hifigan/torch_model.py:221-414 — the discriminator half of the reference's module, forward only, on the HIP library.

``MultiPeriodDiscriminator``, ``MultiScaleDiscriminator``, ``feature_loss``, ``discriminator_loss`` and ``generator_loss`` keep the
reference's names, call signatures and tuple structures; the numbers come from ``viettts_amd.hifigan.discriminators.Discriminators``
(include/vtts_disc.h).  There are no gradients: this is a scoring surface for validation, not a trainer.

Both stacks share one ``Discriminators`` instance per process: either hand one in with ``use_discriminators(d)``, or call
``load_state_dict`` on both modules (upstream's ``do_*`` file: ``mpd.load_state_dict(ckpt["mpd"]); msd.load_state_dict(ckpt["msd"])``).
The loss functions take the lists a discriminator call of this module returned — they read the reduction kernel's results for that
call — and raise ``TypeError`` for anything else: there is no eager fallback.
"""
from __future__ import annotations

from typing import Optional

import torch

from .discriminators import Discriminators, fold_state_dict

LRELU_SLOPE = 0.1
_STATE = {"d": None, "params": {}, "dirty": False}


def use_discriminators(d: Optional[Discriminators]) -> None:
    """Run the module-level surface on ``d`` (already holding its weights); ``None`` forgets it."""
    _STATE.update(d=d, params={}, dirty=False)


def _discriminators() -> Discriminators:
    if _STATE["dirty"]:
        if len(_STATE["params"]) < 54:
            raise RuntimeError("load_state_dict() both MultiPeriodDiscriminator and MultiScaleDiscriminator before the first call")
        if _STATE["d"] is None:
            _STATE["d"] = Discriminators(torch.device("cuda", torch.cuda.current_device()))
        _STATE["d"].load_params(_STATE["params"])
        _STATE.update(params={}, dirty=False)
    if _STATE["d"] is None:
        raise RuntimeError("no weights: load_state_dict() both discriminators, or use_discriminators(d)")
    return _STATE["d"]


class _Call:
    """One 2 B-row pass and, on demand, its reduction."""

    def __init__(self, d: Discriminators, y, y_hat):
        y, y_hat = d._check_input(y), d._check_input(y_hat)
        if y.shape != y_hat.shape:
            raise ValueError(f"y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} must have one shape")
        self.d, (self.B, self.T) = d, y.shape
        self.fb, self.sb = d.forward_raw(torch.cat([y, y_hat]))
        self._raw = None

    @property
    def raw(self) -> torch.Tensor:
        if self._raw is None:
            self._raw = self.d.losses_raw(self.fb, self.sb, self.B, self.T)
        return self._raw


class _Lists(list):
    """A list the reference would return, remembering the call and the stack (0 = MPD, 1 = MSD) it came from."""

    def __init__(self, items, call: _Call, stack: int, role: str):
        super().__init__(items)
        self.call, self.stack, self.role = call, stack, role


class _Stack:
    _prefix, _index, _lo, _hi = "", 0, 0, 0

    def load_state_dict(self, state_dict, strict: bool = True):
        _STATE["params"].update(fold_state_dict(state_dict, self._prefix))
        _STATE["dirty"] = True
        return self

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def forward(self, y, y_hat):
        call = _Call(_discriminators(), y, y_hat)
        scores, fmaps = call.d.views(call.fb, call.sb, 2 * call.B, call.T)
        B, sel = call.B, slice(self._lo, self._hi)
        mk = lambda items, role: _Lists(items, call, self._index, role)  # noqa: E731
        return (mk([s[:B] for s in scores[sel]], "d_r"), mk([s[B:] for s in scores[sel]], "d_g"),
                mk([[m[:B] for m in maps] for maps in fmaps[sel]], "f_r"), mk([[m[B:] for m in maps] for maps in fmaps[sel]], "f_g"))

    __call__ = forward


class MultiPeriodDiscriminator(_Stack):
    """``(y, y_hat) -> y_d_rs, y_d_gs, fmap_rs, fmap_gs`` over the periods 2, 3, 5, 7, 11."""

    _prefix, _index, _lo, _hi = "mpd", 0, 0, 5


class MultiScaleDiscriminator(_Stack):
    """``(y, y_hat) -> y_d_rs, y_d_gs, fmap_rs, fmap_gs`` over the three scales."""

    _prefix, _index, _lo, _hi = "msd", 1, 5, 8


def _same_call(name, *lists_and_roles):
    call, stack = None, None
    for lst, role in lists_and_roles:
        if not isinstance(lst, _Lists) or lst.role != role:
            raise TypeError(f"{name} takes the lists a MultiPeriodDiscriminator / MultiScaleDiscriminator call of this module returned "
                            f"(expected its '{role}' list); there is no eager path for other tensors")
        if call is not None and (lst.call is not call or lst.stack != stack):
            raise TypeError(f"{name}: the lists come from different discriminator calls")
        call, stack = lst.call, lst.stack
    return call, stack


def feature_loss(fmap_r, fmap_g):
    call, stack = _same_call("feature_loss", (fmap_r, "f_r"), (fmap_g, "f_g"))
    return call.raw[78 + stack]


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    call, stack = _same_call("discriminator_loss", (disc_real_outputs, "d_r"), (disc_generated_outputs, "d_g"))
    lo, hi = (0, 5) if stack == 0 else (5, 8)
    raw = call.raw
    return raw[80 + stack], raw[54 + lo : 54 + hi].tolist(), raw[62 + lo : 62 + hi].tolist()


def generator_loss(disc_outputs):
    call, stack = _same_call("generator_loss", (disc_outputs, "d_g"))
    lo, hi = (0, 5) if stack == 0 else (5, 8)
    raw = call.raw
    return raw[82 + stack], [raw[70 + i] for i in range(lo, hi)]
