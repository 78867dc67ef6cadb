// bmpow_host_intake.h -- what the host units that judge received objects share (host only): the header walk
// "QQIvv" and the reference's per-object checks, used by bmpow_intake_batch (bmpow_host_intake.hip) and, for
// the payloads of `object` packets, by bmpow_packets_batch (bmpow_host_packets.hip).  Internal, like bmpow_host.h.
#pragma once
#include "bmpow_host.h"

#include "../../include/bmpow_intake.h"

namespace bmhost {

// The binned kernels' rule for a part of m objects on a device of nbins / 4 CUs (bmpow_host_verify.hip).
bool verify_binned(size_t m, size_t nbins);

// addresses.decodeVarint (src/addresses.py:82-134) over data[0 .. len): false where it raises.
inline bool decode_varint(const uint8_t* p, size_t len, uint64_t& value, size_t& used) {
  value = 0, used = 0;
  if (len == 0) return true;  // "if not data: return (0, 0)"
  const uint8_t f = p[0];
  if (f < 253) {
    value = f, used = 1;
    return true;
  }
  const size_t need = f == 253 ? 3 : f == 254 ? 5 : 9;
  if (len < need) return false;
  uint64_t v = 0;
  for (size_t i = 1; i < need; ++i) v = (v << 8) | p[i];
  const uint64_t least = f == 253 ? 253 : f == 254 ? 65536 : 4294967296ULL;
  if (v < least) return false;  // not the shortest encoding
  value = v, used = need;
  return true;
}

inline int intake_header(const uint8_t* obj, size_t len, bmpow_intake_rec* out) {
  std::memset(out, 0, sizeof(*out));
  if (!obj || len < 20) return 0;  // unpack('>Q' / '>I') of a short slice raises struct.error
  uint64_t version, stream;
  size_t u1, u2;
  if (!decode_varint(obj + 20, len - 20, version, u1)) return 0;
  if (!decode_varint(obj + 20 + u1, len - 20 - u1, stream, u2)) return 0;
  out->nonce = bmsched::load_be64(obj);
  out->expires = bmsched::load_be64(obj + 8);
  out->object_type = ((uint32_t)obj[16] << 24) | ((uint32_t)obj[17] << 16) | ((uint32_t)obj[18] << 8) | obj[19];
  out->version = version;
  out->stream = stream;
  out->payload_offset = (uint32_t)(20 + u1 + u2);
  return 1;
}

inline int intake_status(const bmpow_intake_rec* r, size_t len, int pow_ok, int64_t now, const uint64_t* streams,
                         size_t n_streams) {
  if (!r || r->payload_offset < 20 || r->payload_offset > len) return BMPOW_INTAKE_MALFORMED;
  if (len - r->payload_offset > BMPOW_INTAKE_MAX_PAYLOAD) return BMPOW_INTAKE_TOO_LARGE;  // bmproto.py:386-391
  if (!pow_ok) return BMPOW_INTAKE_INSUFFICIENT_POW;                                    // bmobject.py:71-76
  const __int128 ttl = (__int128)r->expires - (__int128)now;                            // bmobject.py:78-94
  if (ttl > BMPOW_INTAKE_MAX_TTL) return BMPOW_INTAKE_EXPIRED_FUTURE;
  if (ttl < BMPOW_INTAKE_MIN_TTL) return BMPOW_INTAKE_EXPIRED_PAST;
  if (r->stream < 1 || r->stream > 0x7fffffffffffffffULL) return BMPOW_INTAKE_INVALID_STREAM;  // bmobject.py:96-102
  bool wanted = false;
  for (size_t i = 0; i < n_streams && !wanted; ++i) wanted = streams[i] == r->stream;
  if (!wanted) return BMPOW_INTAKE_UNWANTED_STREAM;                                     // bmobject.py:103-107
  switch (r->object_type) {                                                            // bmobject.py:121-163
    case 0: return len < 42 ? BMPOW_INTAKE_INVALID_FOR_TYPE : BMPOW_INTAKE_OK;
    case 1: return len < 146 || len > 440 ? BMPOW_INTAKE_INVALID_FOR_TYPE : BMPOW_INTAKE_OK;
    case 3: return len < 180 || r->version < 2 ? BMPOW_INTAKE_INVALID_FOR_TYPE : BMPOW_INTAKE_OK;
    default: return BMPOW_INTAKE_OK;
  }
}

}  // namespace bmhost
