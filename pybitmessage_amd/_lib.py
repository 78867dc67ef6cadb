"""ctypes binding of ``libbmpow_hip.so`` (C ABI in ``include/bmpow.h``).

Loaded the way the reference loads its native PoW library
(``src/proofofwork.py:371-388``: ``ctypes.CDLL(codePath/bitmsghash/bitmsghash.so)``), but with
``argtypes``/``restype`` set for every entry point.  There is no CPU fallback: if the library
or a gfx950 device is missing, :func:`get` raises :class:`BmpowUnavailable`.
"""
import atexit
import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_PATH = os.path.join(HERE, 'lib', 'libbmpow_hip.so')

NOT_FOUND = 0
FOUND = 1
E_NODEV = -1
E_HIP = -2
E_ARG = -3
E_ABORTED = -4
E_STATE = -5

PENDING = 0
DONE_FOUND = 1
DONE_EXHAUSTED = 2
PARKED = 3
FREE = 4
DONE_BADHASH = 5
SERVICE_VERIFY = 1

U64_MAX = (1 << 64) - 1
MAX_IH_LEN = 1 << 20  # BMPOW_MAX_IH_LEN: longest initialHash the library accepts


class BmpowError(RuntimeError):
    """A libbmpow_hip call failed (HIP error, bad argument, ...)."""

    def __init__(self, code, msg):
        RuntimeError.__init__(self, '%s (code %d)' % (msg, code))
        self.code = code


class BmpowUnavailable(BmpowError):
    """The HIP library is not built or no gfx950 device is visible."""


class BmpowStats(ctypes.Structure):
    _fields_ = [('launches', ctypes.c_uint64), ('trials', ctypes.c_uint64),
                ('kernel_ms', ctypes.c_double), ('max_shard_kernel_ms', ctypes.c_double),
                ('steps', ctypes.c_uint64), ('verify_launches', ctypes.c_uint64),
                ('verify_objects', ctypes.c_uint64), ('verify_blocks', ctypes.c_uint64),
                ('verify_kernel_ms', ctypes.c_double), ('addr_launches', ctypes.c_uint64),
                ('addr_tries', ctypes.c_uint64), ('addr_kernel_ms', ctypes.c_double),
                ('probe_trials', ctypes.c_uint64), ('probe_kernel_ms', ctypes.c_double),
                ('verify_host_build_ms', ctypes.c_double), ('verify_host_run_ms', ctypes.c_double),
                ('verify_host_verdict_ms', ctypes.c_double),
                ('cut_trials', ctypes.c_uint64),
                ('one_wait_spin_ms', ctypes.c_double), ('one_wait_sleep_ms', ctypes.c_double),
                ('past_window', ctypes.c_uint64), ('past_later', ctypes.c_uint64),
                ('past_split', ctypes.c_uint64), ('engine_hashed_est', ctypes.c_uint64),
                ('masked_streams', ctypes.c_uint64), ('run_streams', ctypes.c_uint64)]


class BmpowAddress(ctypes.Structure):
    """``bmpow_address`` (include/bmpow.h): one found try of the address search."""
    _fields_ = [('k', ctypes.c_uint64), ('ripe', ctypes.c_uint8 * 20), ('priv_signing', ctypes.c_uint8 * 32),
                ('priv_encryption', ctypes.c_uint8 * 32), ('pub_signing', ctypes.c_uint8 * 65),
                ('pub_encryption', ctypes.c_uint8 * 65)]


# (name, restype, argtypes) for every symbol include/bmpow.h declares
_u64, _p64, _pu8 = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
_vp = ctypes.c_void_p
_pu32 = ctypes.POINTER(ctypes.c_uint32)
SIGNATURES = [
    ('bmpow_init', ctypes.c_int, []),
    ('bmpow_device_count', ctypes.c_int, []),
    ('bmpow_set_devices', ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    ('bmpow_set_device_count', ctypes.c_int, [ctypes.c_int]),
    ('bmpow_get_devices', ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    ('bmpow_device_pci_bus_id', ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    ('bmpow_get_shard_rates', ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    ('bmpow_shutdown', None, []),
    ('bmpow_atexit', None, []),
    ('bmpow_last_error', ctypes.c_char_p, []),
    ('bmpow_version', ctypes.c_char_p, []),
    ('bmpow_abort', None, []),
    ('bmpow_clear_abort', None, []),
    ('bmpow_trials', ctypes.c_int, [ctypes.c_char_p, _p64, ctypes.c_size_t, _p64]),
    ('bmpow_trials_len', ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, _p64, ctypes.c_size_t, _p64]),
    ('bmpow_search', ctypes.c_int, [ctypes.c_char_p, _u64, _u64, _u64, _p64, _p64]),
    ('bmpow_search_len', ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, _u64, _u64, _u64, _p64, _p64]),
    ('bmpow_min_trial', ctypes.c_int, [ctypes.c_char_p, _u64, _u64, _p64, _p64]),
    ('bmpow_min_trial_batch', ctypes.c_int, [ctypes.c_size_t, ctypes.c_char_p, _p64, _p64, _p64, _p64]),
    ('bmpow_min_trial_var', ctypes.c_int, [ctypes.c_size_t, ctypes.c_char_p, _p64, _p64, _p64, _p64, _p64]),
    ('bmpow_search_batch', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_char_p, _p64, _p64, _u64, _p64, _p64, _pu8]),
    ('bmpow_batch_create', _vp, [ctypes.c_size_t, ctypes.c_char_p, _p64, _p64]),
    ('bmpow_batch_step', ctypes.c_int, [_vp, _u64]),
    ('bmpow_batch_results', ctypes.c_int, [_vp, _p64, _p64, _pu8, _p64]),
    ('bmpow_batch_reset', ctypes.c_int, [_vp, _p64]),
    ('bmpow_batch_set_pending', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]),
    ('bmpow_batch_add', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_char_p, _p64, _p64, _pu32]),
    ('bmpow_batch_add_var', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_char_p, _p64, _p64, _p64, _pu32]),
    ('bmpow_batch_take_done', ctypes.c_int, [_vp, ctypes.c_size_t, _pu32, _p64, _p64, _pu8]),
    ('bmpow_batch_destroy', None, [_vp]),
    ('bmpow_service_create', _vp, [_u64, ctypes.c_uint32]),
    ('bmpow_service_submit', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_char_p, _p64, _p64]),
    ('bmpow_service_submit_var', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_char_p, _p64, _p64, _p64]),
    ('bmpow_service_poll', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_int, _p64, _p64, _p64, _pu8]),
    ('bmpow_service_cancel', ctypes.c_int, [_vp]),
    ('bmpow_service_outstanding', ctypes.c_int, [_vp]),
    ('bmpow_service_stop', None, [_vp]),
    ('bmpow_service_destroy', None, [_vp]),
    ('bmpow_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowStats)]),
    ('bmpow_reset_stats', None, []),
    ('bmpow_get_shard_stats', ctypes.c_int, [_p64, ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    ('bmpow_get_thread_info', ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    ('bmpow_set_shard_throttle', ctypes.c_int, [ctypes.c_int, ctypes.c_double]),
    ('bmpow_set_run_split', ctypes.c_int, [ctypes.c_int]),
    ('bmpow_set_engine_split', ctypes.c_int, [ctypes.c_int]),
    ('bmpow_get_run_pieces', ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    ('bmpow_get_step_trials', _u64, []),
    ('bmpow_set_step_trials', None, [_u64]),
    ('bmpow_pow_values', ctypes.c_int, [ctypes.c_size_t, ctypes.c_char_p, _p64, _p64]),
    ('bmpow_verify_batch', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_char_p, _p64, _p64, _p64, ctypes.POINTER(ctypes.c_int64), _pu8]),
    ('bmpow_verify_batch_ptrs', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, _p64, _p64, ctypes.POINTER(ctypes.c_int64), _pu8]),
    ('bmpow_pow_sufficient', ctypes.c_int, [_u64, _u64, _u64, _u64, ctypes.c_int64, _u64]),
    ('bmpow_vbatch_create', _vp, [ctypes.c_size_t, ctypes.c_char_p, _p64]),
    ('bmpow_vbatch_run', ctypes.c_int, [_vp, _p64]),
    ('bmpow_vbatch_destroy', None, [_vp]),
    ('bmpow_pubkeys', ctypes.c_int, [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]),
    ('bmpow_fe_probe', ctypes.c_int, [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ('bmpow_address_search', ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_size_t, _u64, _u64, ctypes.c_int, ctypes.POINTER(BmpowAddress)]),
    ('bmpow_address_search_random', ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, _u64, _u64, ctypes.c_int, ctypes.POINTER(BmpowAddress)]),
    ('bmpow_addr_set_comb', ctypes.c_int, [ctypes.c_int]),
    ('bmpow_addr_last_comb', ctypes.c_int, []),
    ('BitmessagePOW', ctypes.c_ulonglong, [ctypes.c_char_p, ctypes.c_ulonglong]),
]


class BmpowEciesStats(ctypes.Structure):
    """``bmpow_ecies_stats`` (include/bmpow_ecies.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('objects', ctypes.c_uint64), ('pairs', ctypes.c_uint64),
                ('launches', ctypes.c_uint64), ('prep_ms', ctypes.c_double), ('ecdh_ms', ctypes.c_double),
                ('mac_ms', ctypes.c_double), ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_ecies.h declares
ECIES_SIGNATURES = [
    ('bmpow_ecdh', ctypes.c_int, [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, _pu8, _pu8]),
    ('bmpow_ecies_parse', ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, _pu8, ctypes.POINTER(ctypes.c_size_t)]),
    ('bmpow_ecies_match', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), _pu8]),
    ('bmpow_ecies_decrypt', ctypes.c_int64, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, _pu8, ctypes.c_size_t]),
    ('bmpow_ecies_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowEciesStats)]),
    ('bmpow_ecies_reset_stats', None, []),
]


class BmpowIntakeStats(ctypes.Structure):
    """``bmpow_intake_stats`` (include/bmpow_intake.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('objects', ctypes.c_uint64), ('blocks', ctypes.c_uint64),
                ('launches', ctypes.c_uint64), ('kernel_ms', ctypes.c_double), ('host_build_ms', ctypes.c_double),
                ('host_run_ms', ctypes.c_double), ('host_status_ms', ctypes.c_double)]


class BmpowIntakeRec(ctypes.Structure):
    """``bmpow_intake_rec`` (include/bmpow_intake.h): one object's header fields, hash, POW value and status."""
    _fields_ = [('nonce', ctypes.c_uint64), ('expires', ctypes.c_uint64), ('version', ctypes.c_uint64),
                ('stream', ctypes.c_uint64), ('pow', ctypes.c_uint64), ('object_type', ctypes.c_uint32),
                ('payload_offset', ctypes.c_uint32), ('status', ctypes.c_int32), ('reserved', ctypes.c_uint32),
                ('inv', ctypes.c_uint8 * 32)]


class BmpowIntakeParams(ctypes.Structure):
    """``bmpow_intake_params`` (include/bmpow_intake.h)."""
    _fields_ = [('now', ctypes.c_int64), ('recv_time', ctypes.c_int64), ('ntpb', ctypes.c_uint64),
                ('extra', ctypes.c_uint64), ('streams', _p64), ('n_streams', ctypes.c_size_t)]


# the same for every symbol include/bmpow_intake.h declares
INTAKE_SIGNATURES = [
    ('bmpow_inventory_hashes', ctypes.c_int, [ctypes.c_size_t, ctypes.c_void_p, _p64, _pu8]),
    ('bmpow_intake_header', ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(BmpowIntakeRec)]),
    ('bmpow_intake_status', ctypes.c_int,
     [ctypes.POINTER(BmpowIntakeRec), ctypes.c_size_t, ctypes.c_int, ctypes.c_int64, _p64, ctypes.c_size_t]),
    ('bmpow_intake_batch', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.POINTER(BmpowIntakeParams), ctypes.c_void_p]),
    ('bmpow_intake_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowIntakeStats)]),
    ('bmpow_intake_reset_stats', None, []),
]



class BmpowSigStats(ctypes.Structure):
    """``bmpow_sig_stats`` (include/bmpow_sig.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('submitted', ctypes.c_uint64), ('uploaded', ctypes.c_uint64),
                ('ladders', ctypes.c_uint64), ('launches', ctypes.c_uint64), ('hash_ms', ctypes.c_double),
                ('scalar_ms', ctypes.c_double), ('curve_ms', ctypes.c_double), ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_sig.h declares
SIG_SIGNATURES = [
    ('bmpow_sig_parse', ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, _pu8]),
    ('bmpow_ecdsa_verify_digest', ctypes.c_int, [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, _pu8]),
    ('bmpow_sig_verify', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_void_p, _p64, ctypes.c_char_p, _pu8]),
    ('bmpow_sig_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowSigStats)]),
    ('bmpow_sig_reset_stats', None, []),
]



class BmpowSendStats(ctypes.Structure):
    """``bmpow_send_stats`` (include/bmpow_send.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('rows', ctypes.c_uint64), ('sets', ctypes.c_uint64),
                ('launches', ctypes.c_uint64), ('hash_ms', ctypes.c_double), ('comb_ms', ctypes.c_double),
                ('scalar_ms', ctypes.c_double), ('ladder_ms', ctypes.c_double), ('seal_ms', ctypes.c_double),
                ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_send.h declares
SEND_SIGNATURES = [
    ('bmpow_ec_pubkeys', ctypes.c_int, [ctypes.c_size_t, ctypes.c_char_p, _pu8, _pu8]),
    ('bmpow_ecdsa_sign_digest', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, _pu8, _pu8]),
    ('bmpow_sig_der', ctypes.c_int, [ctypes.c_char_p, _pu8, ctypes.POINTER(ctypes.c_size_t)]),
    ('bmpow_sig_sign', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, _pu8, _pu8]),
    ('bmpow_ecies_seal', ctypes.c_int64,
     [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, _pu8, ctypes.c_size_t]),
    ('bmpow_ecies_encrypt', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, _p64,
      _p64]),
    ('bmpow_send_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowSendStats)]),
    ('bmpow_send_reset_stats', None, []),
]


class BmpowSealStats(ctypes.Structure):
    """``bmpow_seal_stats`` (include/bmpow_send.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('rows_device', ctypes.c_uint64), ('rows_host', ctypes.c_uint64),
                ('sets', ctypes.c_uint64), ('launches', ctypes.c_uint64), ('seal_kernel_ms', ctypes.c_double),
                ('pack_ms', ctypes.c_double), ('copy_ms', ctypes.c_double), ('scatter_ms', ctypes.c_double)]


# the device seal's entry points (include/bmpow_send.h) and the raw CBC call (include/bmpow_ecies.h)
SEAL_SIGNATURES = [
    ('bmpow_ecies_seal_batch', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, _p64,
      _p64]),
    ('bmpow_send_set_seal', ctypes.c_int, [ctypes.c_int]),
    ('bmpow_seal_plan', ctypes.c_int64, [ctypes.c_size_t, _p64, _u64, _u64, _pu32, _p64]),
    ('bmpow_seal_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowSealStats)]),
    ('bmpow_seal_reset_stats', None, []),
    ('bmpow_aes256_cbc', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, _p64, ctypes.c_void_p, _p64,
      ctypes.POINTER(ctypes.c_int64)]),
]


class BmpowIdentRec(ctypes.Structure):
    """``bmpow_ident_rec`` (include/bmpow_ident.h): one row of the sender identification, 180 bytes."""
    _fields_ = [('ripe', ctypes.c_uint8 * 20), ('key_v3', ctypes.c_uint8 * 32), ('tag_key', ctypes.c_uint8 * 32),
                ('tag', ctypes.c_uint8 * 32), ('addr_len', ctypes.c_uint8), ('addr', ctypes.c_char * 63)]


class BmpowIdentStats(ctypes.Structure):
    """``bmpow_ident_stats`` (include/bmpow_ident.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('rows', ctypes.c_uint64), ('sets', ctypes.c_uint64),
                ('launches', ctypes.c_uint64), ('kernel_ms', ctypes.c_double), ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_ident.h declares
IDENT_SIGNATURES = [
    ('bmpow_ident_derive', ctypes.c_int, [ctypes.c_size_t, ctypes.c_void_p, _p64, _p64, ctypes.c_void_p]),
    ('bmpow_ident_from_ripe', ctypes.c_int, [ctypes.c_size_t, ctypes.c_void_p, _p64, _p64, ctypes.c_void_p]),
    ('bmpow_ident_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowIdentStats)]),
    ('bmpow_ident_reset_stats', None, []),
]



class BmpowRxMsgRec(ctypes.Structure):
    """``bmpow_rx_msg_rec`` (include/bmpow_rx.h): one processed msg, 208 bytes."""
    _fields_ = [('sender_version', ctypes.c_uint64), ('sender_stream', ctypes.c_uint64), ('ntpb', ctypes.c_uint64),
                ('extra', ctypes.c_uint64), ('encoding', ctypes.c_uint64), ('claimed_stream', ctypes.c_uint64),
                ('end_of_pubkey', ctypes.c_uint32), ('msg_off', ctypes.c_uint32), ('msg_len', ctypes.c_uint32),
                ('ack_off', ctypes.c_uint32), ('ack_len', ctypes.c_uint32), ('sig_off', ctypes.c_uint32),
                ('sig_len', ctypes.c_uint32), ('bottom', ctypes.c_uint32), ('status', ctypes.c_int32),
                ('ripe', ctypes.c_uint8 * 20), ('sig_hash', ctypes.c_uint8 * 32), ('addr_len', ctypes.c_uint8),
                ('addr', ctypes.c_char * 63), ('behaviour', ctypes.c_uint8 * 4), ('digest', ctypes.c_uint8),
                ('prefix_len', ctypes.c_uint8), ('reserved', ctypes.c_uint8 * 2)]


class BmpowRxStats(ctypes.Structure):
    """``bmpow_rx_stats`` (include/bmpow_rx.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('rows', ctypes.c_uint64), ('sets', ctypes.c_uint64),
                ('launches', ctypes.c_uint64), ('walk_ms', ctypes.c_double), ('hash_ms', ctypes.c_double),
                ('scalar_ms', ctypes.c_double), ('curve_ms', ctypes.c_double), ('ident_ms', ctypes.c_double),
                ('finish_ms', ctypes.c_double), ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_rx.h declares
RX_SIGNATURES = [
    ('bmpow_rx_msgs', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_void_p, _p64, ctypes.c_char_p, ctypes.c_void_p]),
    ('bmpow_rx_walk_msg', ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(BmpowRxMsgRec)]),
    ('bmpow_rx_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowRxStats)]),
    ('bmpow_rx_reset_stats', None, []),
]



class BmpowRxObjRec(ctypes.Structure):
    """``bmpow_rx_obj_rec`` (include/bmpow_rx.h): one processed broadcast or pubkey, 216 bytes."""
    _fields_ = [('object_version', ctypes.c_uint64), ('object_stream', ctypes.c_uint64),
                ('sender_version', ctypes.c_uint64), ('sender_stream', ctypes.c_uint64), ('ntpb', ctypes.c_uint64),
                ('extra', ctypes.c_uint64), ('encoding', ctypes.c_uint64), ('payload_off', ctypes.c_uint32),
                ('tag_off', ctypes.c_uint32), ('end_of_pubkey', ctypes.c_uint32), ('msg_off', ctypes.c_uint32),
                ('msg_len', ctypes.c_uint32), ('sig_off', ctypes.c_uint32), ('sig_len', ctypes.c_uint32),
                ('bottom', ctypes.c_uint32), ('status', ctypes.c_int32), ('ripe', ctypes.c_uint8 * 20),
                ('sig_hash', ctypes.c_uint8 * 32), ('addr_len', ctypes.c_uint8), ('addr', ctypes.c_char * 63),
                ('behaviour', ctypes.c_uint8 * 4), ('digest', ctypes.c_uint8), ('prefix_len', ctypes.c_uint8),
                ('kind', ctypes.c_uint8), ('keys_hashed', ctypes.c_uint8)]


# the broadcast and pubkey half of include/bmpow_rx.h; its counters are a second bmpow_rx_stats
RXOBJ_SIGNATURES = [
    ('bmpow_rx_objects', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p, _p64, ctypes.c_void_p, _p64, ctypes.c_char_p, ctypes.c_void_p]),
    ('bmpow_rx_walk_object', ctypes.c_int,
     [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
      ctypes.POINTER(BmpowRxObjRec)]),
    ('bmpow_rx_obj_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowRxStats)]),
    ('bmpow_rx_obj_reset_stats', None, []),
]


class BmpowRxSealedStats(ctypes.Structure):
    """``bmpow_rx_sealed_stats`` (include/bmpow_rxopen.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('rows', ctypes.c_uint64), ('matched', ctypes.c_uint64),
                ('sets', ctypes.c_uint64), ('launches', ctypes.c_uint64), ('rx_launches', ctypes.c_uint64),
                ('bytes_up', ctypes.c_uint64), ('bytes_down', ctypes.c_uint64), ('match_ms', ctypes.c_double),
                ('open_ms', ctypes.c_double), ('walk_ms', ctypes.c_double), ('hash_ms', ctypes.c_double),
                ('scalar_ms', ctypes.c_double), ('curve_ms', ctypes.c_double), ('ident_ms', ctypes.c_double),
                ('finish_ms', ctypes.c_double), ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_rxopen.h declares
RXOPEN_SIGNATURES = [
    ('bmpow_rx_sealed_msgs', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    ('bmpow_rx_sealed_plan', ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t),
      ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]),
    ('bmpow_rx_sealed_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowRxSealedStats)]),
    ('bmpow_rx_sealed_reset_stats', None, []),
]


class BmpowRxObjTables(ctypes.Structure):
    """``bmpow_rx_obj_tables`` (include/bmpow_rxobjopen.h): the three key tables of one call."""
    _fields_ = [('n_trial', ctypes.c_size_t), ('trial_priv32', ctypes.c_char_p), ('trial_ripe20', ctypes.c_char_p),
                ('n_tags', ctypes.c_size_t), ('tag32', ctypes.c_char_p), ('tag_priv32', ctypes.c_char_p),
                ('n_needed', ctypes.c_size_t), ('needed_tag32', ctypes.c_char_p), ('needed_priv32', ctypes.c_char_p),
                ('needed_ripe20', ctypes.c_char_p), ('needed_version', ctypes.c_void_p),
                ('needed_stream', ctypes.c_void_p), ('needed_flags', ctypes.c_char_p)]


class BmpowRxSealedObjStats(ctypes.Structure):
    """``bmpow_rx_sealed_obj_stats`` (include/bmpow_rxobjopen.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('rows', ctypes.c_uint64), ('matched', ctypes.c_uint64),
                ('clear', ctypes.c_uint64), ('sets', ctypes.c_uint64), ('launches', ctypes.c_uint64),
                ('rx_launches', ctypes.c_uint64), ('tagged_tries', ctypes.c_uint64), ('trial_tries', ctypes.c_uint64),
                ('bytes_up', ctypes.c_uint64), ('bytes_down', ctypes.c_uint64), ('match_ms', ctypes.c_double),
                ('open_ms', ctypes.c_double), ('walk_ms', ctypes.c_double), ('hash_ms', ctypes.c_double),
                ('scalar_ms', ctypes.c_double), ('curve_ms', ctypes.c_double), ('ident_ms', ctypes.c_double),
                ('finish_ms', ctypes.c_double), ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_rxobjopen.h declares
RXOBJOPEN_SIGNATURES = [
    ('bmpow_rx_sealed_objects', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p, _p64, ctypes.POINTER(BmpowRxObjTables), ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    ('bmpow_rx_sealed_object_plan', ctypes.c_int,
     [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t),
      ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t),
      ctypes.POINTER(ctypes.c_int)]),
    ('bmpow_rx_sealed_obj_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowRxSealedObjStats)]),
    ('bmpow_rx_sealed_obj_reset_stats', None, []),
]


class BmpowTxRec(ctypes.Structure):
    """``bmpow_tx_rec`` (include/bmpow_tx.h): one built object, 152 bytes."""
    _fields_ = [('status', ctypes.c_int32), ('obj_len', ctypes.c_uint32), ('plain_len', ctypes.c_uint32),
                ('sig_len', ctypes.c_uint8), ('kind', ctypes.c_uint8), ('digest', ctypes.c_uint8),
                ('reserved', ctypes.c_uint8), ('sig', ctypes.c_uint8 * 72), ('initial_hash', ctypes.c_uint8 * 64)]


class BmpowTxLayout(ctypes.Structure):
    """``bmpow_tx_layout`` (include/bmpow_tx.h)."""
    _fields_ = [('slot_bytes', ctypes.c_uint64), ('body_at', ctypes.c_uint32), ('tail_at', ctypes.c_uint32),
                ('plain_cap', ctypes.c_uint32), ('signed_len', ctypes.c_uint32), ('hash_blocks', ctypes.c_uint32),
                ('reserved', ctypes.c_uint32)]


class BmpowTxStats(ctypes.Structure):
    """``bmpow_tx_stats`` (include/bmpow_tx.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('rows', ctypes.c_uint64), ('sets', ctypes.c_uint64),
                ('launches', ctypes.c_uint64), ('pack_ms', ctypes.c_double), ('hash_ms', ctypes.c_double),
                ('sign_ms', ctypes.c_double), ('ladder_ms', ctypes.c_double), ('seal_ms', ctypes.c_double),
                ('finish_ms', ctypes.c_double), ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_tx.h declares
TX_SIGNATURES = [
    ('bmpow_tx_objects', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, _p64, ctypes.c_char_p,
      ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, _p64,
      ctypes.c_void_p]),
    ('bmpow_tx_layout_row', ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(BmpowTxLayout)]),
    ('bmpow_tx_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowTxStats)]),
    ('bmpow_tx_reset_stats', None, []),
]

class BmpowPacketRec(ctypes.Structure):
    """``bmpow_packet_rec`` (include/bmpow_packets.h): one framed packet, 120 bytes."""
    _fields_ = [('conn', ctypes.c_uint32), ('offset', ctypes.c_uint32), ('length', ctypes.c_uint32),
                ('command', ctypes.c_uint8), ('exact', ctypes.c_uint8), ('reserved', ctypes.c_uint16),
                ('checksum', ctypes.c_uint32), ('computed', ctypes.c_uint32), ('status', ctypes.c_uint32),
                ('reserved2', ctypes.c_uint32), ('intake', BmpowIntakeRec)]


class BmpowPacketConn(ctypes.Structure):
    """``bmpow_packet_conn`` (include/bmpow_packets.h): where one connection's walk stands."""
    _fields_ = [('consumed', ctypes.c_uint64), ('first', ctypes.c_uint32), ('count', ctypes.c_uint32),
                ('close', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


class BmpowPacketsStats(ctypes.Structure):
    """``bmpow_packets_stats`` (include/bmpow_packets.h)."""
    _fields_ = [('calls', ctypes.c_uint64), ('packets', ctypes.c_uint64), ('object_rows', ctypes.c_uint64),
                ('sum_rows', ctypes.c_uint64), ('host_rows', ctypes.c_uint64), ('empty_rows', ctypes.c_uint64),
                ('blocks', ctypes.c_uint64), ('pack_ms', ctypes.c_double), ('object_ms', ctypes.c_double),
                ('sum_ms', ctypes.c_double), ('host_frame_ms', ctypes.c_double), ('host_build_ms', ctypes.c_double),
                ('host_run_ms', ctypes.c_double), ('host_status_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_packets.h declares
PACKETS_SIGNATURES = [
    ('bmpow_packets_frame', ctypes.c_int64,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
      ctypes.POINTER(BmpowPacketConn)]),
    ('bmpow_packets_count', ctypes.c_int64, [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_void_p]),
    ('bmpow_packets_row_blocks', ctypes.c_uint32, [ctypes.c_int, ctypes.c_uint64]),
    ('bmpow_packets_batch', ctypes.c_int64,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_void_p, ctypes.POINTER(BmpowIntakeParams), ctypes.c_void_p,
      ctypes.c_size_t, ctypes.c_void_p]),
    ('bmpow_packets_ack_batch', ctypes.c_int,
     [ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.POINTER(BmpowIntakeParams), ctypes.c_void_p, ctypes.c_void_p]),
    ('bmpow_packets_get_stats', ctypes.c_int, [ctypes.POINTER(BmpowPacketsStats)]),
    ('bmpow_packets_reset_stats', None, []),
]


class BmpowInvValue(ctypes.Structure):
    """``bmpow_inv_value`` (include/bmpow_inv.h): what a set keeps beside a key."""
    _fields_ = [('expires', ctypes.c_uint64), ('stream', ctypes.c_uint32), ('aux', ctypes.c_uint32)]


class BmpowInvPkt(ctypes.Structure):
    """``bmpow_inv_pkt`` (include/bmpow_inv.h): one ``inv`` / ``dinv`` / ``getdata`` payload as walked."""
    _fields_ = [('count', ctypes.c_uint64), ('first_item', ctypes.c_uint32), ('n_items', ctypes.c_uint32),
                ('item_offset', ctypes.c_uint32), ('status', ctypes.c_int32)]


class BmpowInvStats(ctypes.Structure):
    """``bmpow_inv_stats`` (include/bmpow_inv.h)."""
    _fields_ = [('slots', ctypes.c_uint64), ('seed', ctypes.c_uint64), ('live', ctypes.c_uint64),
                ('tombstones', ctypes.c_uint64), ('calls', ctypes.c_uint64), ('rows', ctypes.c_uint64),
                ('launches', ctypes.c_uint64), ('rebuilds', ctypes.c_uint64), ('probes', ctypes.c_uint64),
                ('longest_probe', ctypes.c_uint64), ('lookup_ms', ctypes.c_double), ('claim_ms', ctypes.c_double),
                ('finalize_ms', ctypes.c_double), ('bury_ms', ctypes.c_double), ('rebuild_ms', ctypes.c_double),
                ('list_ms', ctypes.c_double), ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_inv.h declares
INV_SIGNATURES = [
    ('bmpow_invset_create', _vp, [_u64, _u64]),
    ('bmpow_invset_destroy', None, [_vp]),
    ('bmpow_invset_clear', ctypes.c_int, [_vp]),
    ('bmpow_invset_len', ctypes.c_int64, [_vp]),
    ('bmpow_invset_stats', ctypes.c_int, [_vp, ctypes.POINTER(BmpowInvStats)]),
    ('bmpow_invset_add', ctypes.c_int,
     [_vp, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p]),
    ('bmpow_invset_contains', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ('bmpow_invset_remove', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    ('bmpow_invset_sweep', ctypes.c_int64, [_vp, _u64]),
    ('bmpow_invset_list', ctypes.c_int64, [_vp, ctypes.c_uint32, _u64, ctypes.c_void_p, ctypes.c_size_t]),
    ('bmpow_invset_slot', _u64, [_u64, ctypes.c_uint32, ctypes.c_char_p]),
    ('bmpow_inv_walk', ctypes.c_int, [ctypes.c_void_p, _u64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(BmpowInvPkt)]),
    ('bmpow_inv_batch', ctypes.c_int64,
     [_vp, _vp, ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_void_p, _u64, ctypes.c_int, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    ('bmpow_inv_admit', ctypes.c_int,
     [_vp, _vp, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
]


class BmpowProcRec(ctypes.Structure):
    """``bmpow_proc_rec`` (include/bmpow_proc.h): one dispatched object, 72 bytes."""
    _fields_ = [('version', ctypes.c_uint64), ('stream', ctypes.c_uint64), ('port', ctypes.c_uint64),
                ('route', ctypes.c_uint32), ('ack', ctypes.c_uint32), ('ack_aux', ctypes.c_uint32),
                ('ack_first', ctypes.c_uint32), ('status', ctypes.c_uint32), ('key_off', ctypes.c_uint32),
                ('key_len', ctypes.c_uint32), ('address', ctypes.c_uint32), ('host_off', ctypes.c_uint32),
                ('host_len', ctypes.c_uint32), ('host_class', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


class BmpowProcAddress(ctypes.Structure):
    """``bmpow_proc_address`` (include/bmpow_proc.h): one of my addresses, 80 bytes."""
    _fields_ = [('ripe', ctypes.c_uint8 * 20), ('tag', ctypes.c_uint8 * 32), ('version', ctypes.c_uint32),
                ('stream', ctypes.c_uint64), ('last_pubkey_send_time', ctypes.c_int64), ('chan', ctypes.c_uint32),
                ('reserved', ctypes.c_uint32)]


class BmpowProcParams(ctypes.Structure):
    """``bmpow_proc_params`` (include/bmpow_proc.h)."""
    _fields_ = [('now', ctypes.c_int64), ('rows_per_launch', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


class BmpowProcStats(ctypes.Structure):
    """``bmpow_proc_stats`` (include/bmpow_proc.h)."""
    _fields_ = [('seed', ctypes.c_uint64), ('watch_len', ctypes.c_uint64), ('watch_slots', ctypes.c_uint64),
                ('watch_lengths', ctypes.c_uint64), ('addresses', ctypes.c_uint64), ('calls', ctypes.c_uint64),
                ('rows', ctypes.c_uint64), ('rows_uploaded', ctypes.c_uint64), ('ack_rows', ctypes.c_uint64),
                ('bytes_uploaded', ctypes.c_uint64), ('table_uploads', ctypes.c_uint64), ('launches', ctypes.c_uint64),
                ('found', ctypes.c_uint64), ('rows_ms', ctypes.c_double), ('finish_ms', ctypes.c_double),
                ('host_ms', ctypes.c_double)]


# the same for every symbol include/bmpow_proc.h declares
PROC_SIGNATURES = [
    ('bmpow_proc_create', _vp, [_u64, ctypes.c_int]),
    ('bmpow_proc_destroy', None, [_vp]),
    ('bmpow_proc_stats_get', ctypes.c_int, [_vp, ctypes.POINTER(BmpowProcStats)]),
    ('bmpow_proc_stats_reset', ctypes.c_int, [_vp]),
    ('bmpow_proc_watch_add', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_char_p, _p64, ctypes.c_void_p, ctypes.c_void_p]),
    ('bmpow_proc_watch_discard', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_char_p, _p64, ctypes.c_void_p]),
    ('bmpow_proc_watch_contains', ctypes.c_int,
     [_vp, ctypes.c_size_t, ctypes.c_char_p, _p64, ctypes.c_void_p, ctypes.c_void_p]),
    ('bmpow_proc_watch_len', ctypes.c_int64, [_vp]),
    ('bmpow_proc_watch_clear', ctypes.c_int, [_vp]),
    ('bmpow_proc_watch_slot', _u64, [_u64, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]),
    ('bmpow_proc_set_addresses', ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_void_p]),
    ('bmpow_proc_batch', ctypes.c_int,
     [_vp, ctypes.c_size_t, ctypes.c_void_p, _p64, ctypes.c_void_p, ctypes.POINTER(BmpowProcParams), ctypes.c_void_p]),
    ('bmpow_proc_walk', ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_char_p, _u64, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int64,
      ctypes.POINTER(BmpowProcRec)]),
]

_lock = threading.Lock()
_lib = None
_host = None
_exit_hooked = False


def lib_path():
    return os.environ.get('BMPOW_LIB', DEFAULT_PATH)


def load(path=None):
    """dlopen the library and bind every signature (no device access)."""
    path = path or lib_path()
    if not os.path.exists(path):
        raise BmpowUnavailable(E_NODEV, 'libbmpow_hip.so not built at %s (run __graft_entry__.build() '
                                        'or make -C pybitmessage_amd/csrc)' % path)
    lib = ctypes.CDLL(path)
    for name, res, args in (SIGNATURES + ECIES_SIGNATURES + INTAKE_SIGNATURES + SIG_SIGNATURES + SEND_SIGNATURES +
                            SEAL_SIGNATURES + IDENT_SIGNATURES + RX_SIGNATURES + RXOBJ_SIGNATURES + TX_SIGNATURES +
                            RXOPEN_SIGNATURES + RXOBJOPEN_SIGNATURES + PACKETS_SIGNATURES + INV_SIGNATURES +
                            PROC_SIGNATURES):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if os.path.abspath(path) == os.path.abspath(DEFAULT_PATH):
                raise
            continue  # an A/B build of an earlier round (BMPOW_LIB) may lack later entry points
        fn.restype = res
        fn.argtypes = args
    return lib


def get():
    """The initialised library (devices selected).  Raises BmpowUnavailable."""
    global _lib, _exit_hooked
    with _lock:
        if _lib is None:
            lib = load()
            rc = lib.bmpow_init()
            if rc <= 0:
                raise BmpowUnavailable(rc, 'bmpow_init failed: %s' % lib.bmpow_last_error().decode())
            _lib = lib
            if not _exit_hooked:
                # release the devices (service threads, stepper threads, the streams kept for the
                # process) while the interpreter is still whole; the library's own C atexit hook then
                # finds nothing left to do
                atexit.register(_at_exit, lib)
                _exit_hooked = True
        return _lib


def host():
    """The library for its host-only entry points (``bmpow_ecies_parse``, ``bmpow_ecies_decrypt``, ...):
    the initialised handle when there is one, else a handle loaded without touching a device."""
    global _host
    with _lock:
        if _lib is not None:
            return _lib
        if _host is None:
            _host = load()
        return _host


def _at_exit(lib):
    """Python's exit: ``bmpow_atexit`` (include/bmpow.h) before the HIP runtime's exit handlers."""
    fn = getattr(lib, 'bmpow_atexit', None)
    if fn is not None:
        fn()


def reset():
    """Forget the loaded handle's device selection (``resetPoW``)."""
    global _lib
    with _lock:
        if _lib is not None:
            _lib.bmpow_shutdown()
            _lib = None


def check(lib, rc, what):
    if rc < 0:
        msg = lib.bmpow_last_error().decode(errors='replace')
        if rc == E_NODEV:
            raise BmpowUnavailable(rc, '%s: %s' % (what, msg))
        raise BmpowError(rc, '%s: %s' % (what, msg))
    return rc


def u64_array(values):
    arr = (ctypes.c_uint64 * len(values))()
    for i, v in enumerate(values):
        arr[i] = v
    return arr
