"""Retry tokens of a server, sealed with AES-128-GCM under a key of its own.

The surface is the reference's QuicRetryTokenHandler (quic/retry.py):
create_token(addr, original_destination_connection_id,
retry_source_connection_id) and validate_token(addr, token) -> (odcid,
retry_scid), ValueError for a token that is not ours.  The token's plaintext
is the reference's buffer, three opaques with a one-byte length: the encoded
address (encode_address: the packed IP, then the port big-endian), the
original DCID and the Retry's source CID.  Where the reference wraps it with
RSA-OAEP, a token here is

    counter (8 bytes, big-endian) | AEAD(plaintext, aad = counter, pn = counter)

so the device can seal a whole batch of them in one qpp_protect launch
(qpp_route_reply: the same bytes, receive.answer_routed), and one AEAD.decrypt
validates one.  The token is opaque to the client and private to the server,
so its form is ours to choose (RFC 9000 sec. 8.1.2).  The counter makes every
(key, nonce) pair unique: take(n) hands out n consecutive values, to
create_token and to the device alike, and never the same value twice.

RetryTokens also holds the 3-slot key table the device's two reply launches
use (layout.RP_SLOT_*): the Retry integrity keys of RFC 9001 sec. 5.8 and
RFC 9369 sec. 3.3.3, and the token key.
"""

from __future__ import annotations

import ipaddress
import os
import socket
import threading
from typing import Optional, Tuple

import numpy as np

from . import layout as L
from .packet import (RETRY_AEAD_KEY_VERSION_1, RETRY_AEAD_KEY_VERSION_2, RETRY_AEAD_NONCE_VERSION_1,
                     RETRY_AEAD_NONCE_VERSION_2)

__all__ = ["RetryTokens", "encode_address", "packed_address"]

_CTR = 8
_TAG = 16


def encode_address(addr) -> bytes:
    """quic/retry.py:11-12: the packed IP address, then the port big-endian."""
    host = addr[0]
    try:  # the same bytes as ipaddress gives, without building its object per datagram
        packed = socket.inet_pton(socket.AF_INET6 if ":" in host else socket.AF_INET, host)
    except (OSError, TypeError):
        packed = ipaddress.ip_address(host).packed
    return packed + bytes([addr[1] >> 8, addr[1] & 0xFF])


def packed_address(addr) -> bytes:
    """One candidate's layout.RP_ADDR_STRIDE bytes for qpp_route_reply: the
    length of encode_address(addr) (6 or 18), its bytes, zero padding."""
    e = encode_address(addr)
    return bytes([len(e)]) + e + bytes(L.RP_ADDR_STRIDE - 1 - len(e))


def _opaque(b: bytes) -> bytes:
    if len(b) > 255:
        raise ValueError("an opaque of more than 255 bytes")
    return bytes([len(b)]) + bytes(b)


class RetryTokens:
    def __init__(self, key: Optional[bytes] = None, iv: Optional[bytes] = None, *, counter: int = 0):
        self.key = os.urandom(16) if key is None else bytes(key)
        self.iv = os.urandom(12) if iv is None else bytes(iv)
        if len(self.key) != 16 or len(self.iv) != 12:
            raise ValueError("the token key is 16 bytes and its IV 12 (AES-128-GCM)")
        self._next = int(counter)
        self._lock = threading.Lock()
        self._aead = None
        self._table = None

    # ------------------------------------------------------------ keys ----

    def key_records(self) -> np.ndarray:
        """The reply table's three layout.KEY_MATERIAL records."""
        return np.concatenate([
            L.key_material(L.RP_SLOT_V1, L.AES_128_GCM, RETRY_AEAD_KEY_VERSION_1, RETRY_AEAD_NONCE_VERSION_1, b""),
            L.key_material(L.RP_SLOT_V2, L.AES_128_GCM, RETRY_AEAD_KEY_VERSION_2, RETRY_AEAD_NONCE_VERSION_2, b""),
            L.key_material(L.RP_SLOT_TOKEN, L.AES_128_GCM, self.key, self.iv, b""),
        ])

    @property
    def table(self):
        """The device key table of the two reply launches, made on first use."""
        if self._table is None:
            from . import _crypto

            table = _crypto.KeyTable(3)
            table.set(self.key_records().tobytes())
            self._table = table
        return self._table

    def _cipher(self):
        if self._aead is None:
            from ._crypto import AEAD

            self._aead = AEAD(b"aes-128-gcm", self.key, self.iv)
        return self._aead

    # -------------------------------------------------------- counters ----

    def take(self, n: int) -> int:
        """The first of n consecutive counters nobody else gets."""
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        with self._lock:
            first = self._next
            if first + n >= 1 << 64:  # the device form's rule: token_ctr + n does not wrap
                raise OverflowError("the token counter is used up: change the key")
            self._next = first + n
        return first

    # ---------------------------------------------------------- tokens ----

    @staticmethod
    def plaintext(addr, original_destination_connection_id: bytes, retry_source_connection_id: bytes) -> bytes:
        """create_token's buffer (quic/retry.py:25-28)."""
        return (_opaque(encode_address(addr)) + _opaque(original_destination_connection_id)
                + _opaque(retry_source_connection_id))

    def seal(self, counter: int, addr, original_destination_connection_id: bytes,
             retry_source_connection_id: bytes) -> bytes:
        """The token for a counter the caller took: what the device builds for
        token_ctr + a == counter."""
        head = int(counter).to_bytes(_CTR, "big")
        body = self.plaintext(addr, original_destination_connection_id, retry_source_connection_id)
        return head + self._cipher().encrypt(body, head, int(counter))

    def create_token(self, addr, original_destination_connection_id: bytes,
                     retry_source_connection_id: bytes) -> bytes:
        return self.seal(self.take(1), addr, original_destination_connection_id, retry_source_connection_id)

    def validate_token(self, addr, token: bytes) -> Tuple[bytes, bytes]:
        from ._crypto import CryptoError

        token = bytes(token)
        if len(token) < _CTR + 3 + _TAG:
            raise ValueError("Retry token is too short.")
        counter = int.from_bytes(token[:_CTR], "big")
        try:
            body = self._cipher().decrypt(token[_CTR:], token[:_CTR], counter)
        except CryptoError:
            raise ValueError("Retry token does not authenticate.") from None
        fields, at = [], 0
        for _ in range(3):
            if at >= len(body) or at + 1 + body[at] > len(body):
                raise ValueError("Retry token is malformed.")
            fields.append(body[at + 1:at + 1 + body[at]])
            at += 1 + body[at]
        if fields[0] != encode_address(addr):
            raise ValueError("Remote address does not match.")
        return fields[1], fields[2]
