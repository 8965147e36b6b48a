"""The routed-send restatement against the project's own packet builder.

tests/send_cases.py restates the reference's builder for a 1-RTT packet; the
device lane is held to it (tests/test_send_host.py, tests/test_gpu_send.py).
Here the restatement itself is held to aioquic_amd.packet_builder: for the
same peer CID, spin bit, key phase and packet number its header equals the
bytes QuicPacketBuilder._write_header leaves and its padding equals
_padding_for, compared on the plaintext datagrams of _close(); and the
datagrams of flush(), protected by the oracle stand-in of
tests/test_packet_builder_batched.py, equal the oracle's protection of
restated header || payload || padding.  CPU only.
"""

import numpy as np
import pytest

from aioquic_amd import layout as L
from aioquic_amd import packet_builder as PB
from aioquic_amd.packet import QuicFrameType, QuicPacketType, QuicProtocolVersion
from tests import send_cases as S
from tests.test_packet_builder_batched import _Ctx, _oracle_protect

KEY_LEN = S.KEY_LEN


class _Pair:
    aead_tag_size = 16
    _update_key_requested = False

    def __init__(self, suite, phase, seed):
        rng = np.random.default_rng(seed)
        kl = KEY_LEN[suite]
        self.send = _Ctx(suite, rng.bytes(kl), rng.bytes(12), rng.bytes(kl), phase)

    @property
    def key_phase(self):
        return self.send.key_phase


def _payload(rng, size):
    # one STREAM frame's bytes: the builder writes the frame type itself
    return bytes([QuicFrameType.STREAM_BASE]) + rng.bytes(size - 1)


CASES = [(suite, cid_len, phase, spin, pn)
         for suite in (L.AES_128_GCM, L.AES_256_GCM, L.CHACHA20_POLY1305)
         for cid_len, phase, spin, pn in ((0, 0, 0, 0), (1, 1, 1, 0xFFFE), (8, 1, 0, (1 << 32) + 0xFFFD),
                                          (20, 0, 1, (1 << 40) + 5))]


@pytest.mark.parametrize("suite,cid_len,phase,spin,pn", CASES)
def test_header_and_padding_match_the_builder(oracle, monkeypatch, suite, cid_len, phase, spin, pn):
    rng = np.random.default_rng(1000 * suite + cid_len)
    cid = rng.bytes(cid_len)
    pair = _Pair(suite, phase, seed=pn & 0xFFFF)
    sizes = [1, 2, 3, 1173, S.longest_payload(cid_len)]
    payloads = [_payload(rng, size) for size in sizes]

    def build():
        b = PB.QuicPacketBuilder(host_cid=bytes(8), peer_cid=cid, version=QuicProtocolVersion.VERSION_1,
                                 is_client=False, max_datagram_size=1500, packet_number=pn, spin_bit=bool(spin))
        for p in payloads:
            b.start_packet(QuicPacketType.ONE_RTT, pair)
            b.start_frame(QuicFrameType.STREAM_BASE, capacity=len(p)).push_bytes(p[1:])
        return b

    # ---- plaintext: what _write_header and _padding_for leave
    b = build()
    plains, pending, packets = b._close()
    assert len(plains) == len(payloads) and b.packet_number == pn + len(payloads)
    restated = []
    for k, (plain, p) in enumerate(zip(plains, payloads)):
        hdr = S.short_header(spin, phase, cid, pn + k)
        pad = S.padding_size(len(p))
        assert len(hdr) == S.header_size(cid_len)
        assert plain == hdr + p + bytes(pad) + bytes(16), (k, len(p))
        assert packets[k].packet_number == pn + k and packets[k].sent_bytes == len(plain)
        restated.append((hdr, p + bytes(pad)))
    assert S.padding_size(1) == 1 and S.padding_size(2) == 0
    assert [(hs, size - hs) for _, _, hs, size, _, _ in pending.packets()] == \
        [(len(h), len(body)) for h, body in restated]
    # ---- protected: flush() through the oracle stand-in
    monkeypatch.setattr(PB, "_protect_datagrams", _oracle_protect(oracle))
    wires, _ = build().flush()
    s = pair.send
    key, iv = s.aead._material()[1:]
    hp = s.hp._material()[1]
    assert wires == [oracle.protect(suite, key, iv, hp, h, body, pn + k) for k, (h, body) in enumerate(restated)]


def test_restated_descriptor_is_the_builders_pending_entry():
    """restate()'s descriptor of an OK packet says what the builder's _Pending
    says: header size, header + payload + padding size, packet number."""
    w = S.World(257, fused=True)
    _, desc, rec = S.restate_world(w)
    ok = rec["status"] == L.SN_OK
    assert ok.sum() > 200
    for i in np.flatnonzero(ok)[:64]:
        c = w.conns[w.conn[i]]
        hs = 1 + int(c["cid_len"]) + PB.PACKET_NUMBER_SEND_SIZE
        pad = max(0, PB.PACKET_NUMBER_MAX_SIZE - PB.PACKET_NUMBER_SEND_SIZE - int(w.len[i]))
        assert (desc["hdr_len"][i], desc["len"][i]) == (hs, int(w.len[i]) + pad)
        assert desc["pn"][i] == int(c["next_pn"]) + int(w.seq[i]) and desc["in_off"][i] == int(w.off[i]) - hs
