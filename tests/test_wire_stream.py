"""wire.start_stream: the ClusterState messages of one cluster's Start stream
(trader_server.go:24-47) from a row of Engine.cluster_state_series and the record at its first
sample.  CPU only; the bytes are derived by hand."""
import numpy as np

from mcs_amd import CLUSTER_SAMPLE_DTYPE, CLUSTER_STATE_DTYPE
from mcs_amd import wire as W


def test_start_stream_bytes():
    """Two samples of one cluster, totals (320, 240000), average wait 1.5 ms.

    Message 0 (the first after a cluster change carries the totals, trader_server.go:28-34):
      field 1 float 0.75  = 0x3f400000 -> 0d 0000403f
      field 2 float 0.125 = 0x3e000000 -> 15 0000003e
      field 3 varint 320  = 0x140: 0x40|0x80, 0x02 -> 18 c002
      field 4 varint 240000 = 0x3a980: 0x00|0x80, 0x53|0x80, 0x0e -> 20 80d30e
      field 5 double 1.5  = 0x3ff8000000000000 -> 29 000000000000f83f
    Message 1 (no totals; memory utilization 0.0 has implicit presence and is omitted):
      field 1 float 1.0   = 0x3f800000 -> 0d 0000803f
      field 5 double 1.5  -> 29 000000000000f83f
    running and queued are telemetry of the series, not fields of pb.ClusterState."""
    samples = np.array([(0.75, 0.125, 7, 2), (1.0, 0.0, 9, 0)], CLUSTER_SAMPLE_DTYPE)
    first = np.array([(0.75, 0.125, 320, 240000, 7, 40)], CLUSTER_STATE_DTYPE)[0]
    msgs = W.start_stream(samples, first, avg_wait_ms=1.5)
    assert len(msgs) == 2
    raw = [W.marshal(m) for m in msgs]
    assert raw[0].hex() == "0d0000403f150000003e18c0022080d30e29000000000000f83f"
    assert raw[1].hex() == "0d0000803f29000000000000f83f"
    # fields 3 and 4 (tags 0x18, 0x20) only on the first message
    assert b"\x18\xc0\x02\x20\x80\xd3\x0e" in raw[0]
    back = [W.unmarshal(W.ClusterState, r) for r in raw]
    assert back == msgs
    assert (back[0].total_cpu, back[0].total_memory) == (320, 240000)
    assert back[1].total_cpu is None and back[1].total_memory is None
    assert back[1].cores_utilization == 1.0 and back[1].average_wait_time == 1.5


def test_start_stream_default_wait_and_empty_row():
    samples = np.array([(0.5, 0.25, 1, 0)], CLUSTER_SAMPLE_DTYPE)
    first = np.array([(0.5, 0.25, 160, 120000, 1, 0)], CLUSTER_STATE_DTYPE)[0]
    (m,) = W.start_stream(samples, first)
    # the bytes of tests/test_wire.py's first record: average_wait_time 0.0 is omitted
    assert W.marshal(m).hex() == "0d0000003f150000803e18a00120c0a907"
    assert W.start_stream(samples[:0], first) == []
