"""The condition tests/test_graph_handover_gpu.py's part A rests on, on the CPU
backend alone: every eager window of its schedule holds random restarts, so a
stale step key in that window would change the state."""
import handover_cases as hc


def test_schedule_eager_windows_hold_restarts():
    import skillshot_learning_amd as ssa
    ssa.load_library()
    windows = hc.a_reference_windows(ssa)
    assert [w[0] for w in windows] == [call for _, call, _ in hc.A_SCHEDULE]
    hc.assert_a_condition(windows)
