"""The low-latency switch of the text -> mel surface without a GPU: set_low_latency() only stores a flag (the acoustic model is created lazily, on the
first predict_mel), the CLI's --low-latency flag parses, and the reference-named package re-exports the switch."""
from viettts_amd.nat import text2mel as t2m
from viettts_amd.synthesizer import build_parser


def test_set_low_latency_only_stores_the_flag():
    assert t2m._ACOUSTIC_MODEL is None
    was = t2m.get_low_latency()
    try:
        assert was is False  # off by default
        t2m.set_low_latency(True)
        assert t2m.get_low_latency() is True and t2m._ACOUSTIC_MODEL is None  # nothing was created
        t2m.set_low_latency(False)
        assert t2m.get_low_latency() is False
    finally:
        t2m.set_low_latency(was)


def test_flag_is_applied_to_an_installed_model_and_on_toggle():
    class Model:
        def __init__(self):
            self.options = []

        def set_option(self, key, value):
            self.options.append((key, value))

    m = Model()
    was = t2m.get_low_latency()
    try:
        t2m.set_low_latency(True)
        t2m.set_acoustic_model(m)  # installed while the flag is on
        t2m.set_low_latency(False)  # toggled while a model is cached
        t2m.set_low_latency(True)
        assert m.options == [("resident", 1), ("resident", 0), ("resident", 1)]
    finally:
        t2m.set_acoustic_model(None)
        t2m.set_low_latency(was)


def test_cli_low_latency_flag_parses():
    p = build_parser()
    assert p.parse_args(["--text", "xin chào"]).low_latency is False
    a = p.parse_args(["--text", "xin chào", "--low-latency"])
    assert a.low_latency is True and a.mel_file is None


def test_reference_named_package_reexports_the_switch():
    from vietTTS.nat import text2mel as ref_named

    assert ref_named.set_low_latency is t2m.set_low_latency
