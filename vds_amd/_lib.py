"""ctypes loader for libvds_ec.so (the C ABI in include/vds_ec.h).

The library is built in-tree by vds_amd/build.py.  There is no CPU fallback:
if the shared object is missing or no GPU is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VDS_EC_LIB") or os.path.join(HERE, "libvds_ec.so")

OK = 0
EINVAL = -1
ENODEV = -2
ENOMEM = -3
ESINGULAR = -4
ERESTORE = -5
EHIP = -6
EB64_LENGTH = -7
EB64_PADDING = -8
EB64_CHAR = -9
ECORRUPT = -10
EDGRAM_SIGNATURE = -11
EDGRAM_DATA = -12
EDGRAM_INCOMPLETE = -13
EWS_SHORT = -14
EWS_FRAME = -15
EWS_FORM = -16
EWS_PING = -17
ECRYPT_LENGTH = -18
ECRYPT_PADDING = -19
EINFLATE_DATA = -20
EINFLATE_SHORT = -21
EINFLATE_SPACE = -22
ETX_FORM = -23
ETX_KEY = -24

F_NO_TRAILER = 0x1
F_CELLS = 0x2

# Every entry point include/vds_ec.h declares, with its ctypes signature.
u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)
u64p = C.POINTER(C.c_uint64)
vpp = C.POINTER(C.c_void_p)
u32p = C.POINTER(C.c_uint32)


class DgramMessage(C.Structure):
    """vds_ec_dgram_message (include/vds_ec.h)."""
    _fields_ = [("session", C.c_uint32), ("index0", C.c_uint32), ("dgrams", C.c_uint32), ("type", C.c_uint32),
                ("status", C.c_int32), ("route_len", C.c_uint32), ("route_off", C.c_uint64),
                ("msg_off", C.c_uint64), ("msg_len", C.c_uint64)]


class WsFrame(C.Structure):
    """vds_ec_ws_frame (include/vds_ec.h)."""
    _fields_ = [("fin", C.c_uint8), ("rsv1", C.c_uint8), ("rsv2", C.c_uint8), ("rsv3", C.c_uint8),
                ("opcode", C.c_uint8), ("masked", C.c_uint8), ("mask", C.c_uint8 * 4), ("header_len", C.c_uint32),
                ("need", C.c_uint32), ("payload_len", C.c_uint64)]


class RsaKey(C.Structure):
    """vds_ec_rsa_key (include/vds_ec.h)."""
    _fields_ = [("n", C.c_uint32 * 128), ("rr", C.c_uint32 * 128), ("limbs", C.c_uint32), ("n_bytes", C.c_uint32),
                ("e", C.c_uint32), ("n0inv", C.c_uint32)]


class TxBlock(C.Structure):
    """vds_ec_txblock (include/vds_ec.h)."""
    _fields_ = [(f, C.c_uint64) for f in ("time_point", "order_no", "key_id_off", "key_id_len", "ancestors_off",
                                          "ancestors_len", "ancestors_count", "messages_off", "messages_len",
                                          "signature_off", "signature_len", "signed_len")]


i32p = C.POINTER(C.c_int32)

SIGNATURES = {
    "vds_ec_strerror": (C.c_char_p, [C.c_int]),
    "vds_ec_version": (C.c_int, []),
    "vds_ec_host_ctx_stats": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vds_ec_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "vds_ec_replica_size": (C.c_uint64, [C.c_uint, C.c_uint, C.c_uint64, C.c_uint]),
    "vds_ec_restored_size": (C.c_uint64, [C.c_uint, C.c_uint, C.c_uint64, C.c_uint16]),
    "vds_ec_gf16_tables": (C.c_int, [u16p, u16p]),
    "vds_ec_gf8_tables": (C.c_int, [u8p, u8p]),
    "vds_ec_multipliers16": (C.c_int, [C.c_uint16, C.c_uint16, u16p]),
    "vds_ec_multipliers8": (C.c_int, [C.c_uint8, C.c_uint8, u8p]),
    "vds_ec_inverse16": (C.c_int, [C.c_uint16, u16p, u16p]),
    "vds_ec_inverse8": (C.c_int, [C.c_uint8, u8p, u8p]),
    "vds_ec_encode16_device": (C.c_int, [C.c_uint16, u16p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                                         C.c_uint32, vpp, C.c_uint64, C.c_uint, C.c_void_p]),
    "vds_ec_encode8_device": (C.c_int, [C.c_uint8, u8p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                                        C.c_uint32, vpp, C.c_uint64, C.c_uint, C.c_void_p]),
    "vds_ec_restore16_device": (C.c_int, [C.c_uint16, u16p, vpp, C.c_uint64, C.c_uint64, C.c_uint16,
                                          C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint, C.c_void_p]),
    "vds_ec_restore8_device": (C.c_int, [C.c_uint8, u8p, vpp, C.c_uint64, C.c_uint64, C.c_uint16,
                                         C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint, C.c_void_p]),
    "vds_ec_encode16_host": (C.c_int, [C.c_uint16, u16p, C.c_uint32, C.c_void_p, C.c_uint64, vpp, C.c_uint]),
    "vds_ec_encode8_host": (C.c_int, [C.c_uint8, u8p, C.c_uint32, C.c_void_p, C.c_uint64, vpp, C.c_uint]),
    "vds_ec_restore16_host": (C.c_int, [C.c_uint16, u16p, vpp, C.c_uint64, C.c_void_p, u64p, C.c_uint]),
    "vds_ec_restore8_host": (C.c_int, [C.c_uint8, u8p, vpp, C.c_uint64, C.c_void_p, u64p, C.c_uint]),
    "vds_ec_host_alloc": (C.c_int, [C.c_uint64, C.POINTER(C.c_void_p)]),
    "vds_ec_host_free": (C.c_int, [C.c_void_p]),
    "vds_ec_host_register": (C.c_int, [C.c_void_p, C.c_uint64]),
    "vds_ec_host_unregister": (C.c_int, [C.c_void_p]),
    "vds_ec_encode16_host_batch": (C.c_int, [C.c_uint16, u16p, C.c_uint32, vpp, u64p, C.c_uint32, vpp,
                                             C.c_uint, C.c_int]),
    "vds_ec_restore16_host_batch": (C.c_int, [C.c_uint16, u16p, vpp, u64p, C.c_uint32, vpp, u64p, C.c_uint, C.c_int]),
    "vds_ec_regenerate16_device": (C.c_int, [C.c_uint16, u16p, vpp, C.c_uint64, C.c_uint64, C.c_uint32, u16p,
                                             C.c_uint32, vpp, C.c_uint64, C.c_void_p]),
    "vds_ec_regenerate16_host": (C.c_int, [C.c_uint16, u16p, vpp, C.c_uint64, u16p, C.c_uint32, vpp]),
    "vds_ec_regenerate16_path": (C.c_int, [C.c_uint16, u16p, u16p, C.c_uint32, C.c_uint64]),
    "vds_ec_sha256_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "vds_ec_sha256_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "vds_ec_encode16_hash_host": (C.c_int, [C.c_uint16, u16p, C.c_uint32, C.c_void_p, C.c_uint64, vpp, C.c_void_p,
                                            C.c_uint]),
    "vds_ec_replica_paths": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "vds_ec_fill_splitmix_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "vds_ec_encode16_path": (C.c_int, [C.c_uint16, u16p, C.c_uint32, C.c_uint64]),
    "vds_ec_restore16_path": (C.c_int, [C.c_uint16, u16p, C.c_uint64, C.c_uint16, C.c_uint32]),
    "vds_ec_jit_set_mode": (C.c_int, [C.c_int]),
    "vds_ec_jit_wait": (C.c_int, []),
    "vds_ec_jit_build16": (C.c_int, [C.c_uint16, u16p, u64p]),
    "vds_ec_jit_ready16": (C.c_int, [C.c_uint16, u16p]),
    "vds_ec_jit_dump16": (C.c_int, [C.c_uint16, u16p, C.c_int, C.c_char_p]),
    "vds_ec_restore16_batch_device": (C.c_int, [C.c_uint16, C.c_uint32, u16p, vpp, u64p, u16p, vpp, C.c_uint,
                                                C.c_void_p]),
    "vds_ec_regenerate16_batch_device": (C.c_int, [C.c_uint16, C.c_uint32, u16p, vpp, u64p, C.c_uint32, u16p, vpp,
                                                   C.c_void_p]),
    "vds_ec_encode16_batch_device": (C.c_int, [C.c_uint16, u16p, C.c_uint32, C.c_uint32, vpp, u64p, vpp, C.c_uint,
                                               C.c_void_p]),
    "vds_ec_encode16_batch_path": (C.c_int, [C.c_uint16, u16p, C.c_uint32, C.c_uint32, vpp, u64p, vpp, C.c_uint,
                                             C.POINTER(C.c_uint32)]),
    "vds_ec_sha256_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p]),
    "vds_ec_save_temp16_batch_device": (C.c_int, [C.c_uint16, C.c_uint32, C.c_uint32, vpp, u64p, vpp, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    "vds_ec_save_temp16_host_batch": (C.c_int, [C.c_uint16, C.c_uint32, C.c_uint32, vpp, u64p, vpp, C.c_void_p,
                                                C.c_void_p, C.POINTER(C.c_uint32)]),
    "vds_ec_sha256_check_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]),
    "vds_ec_repair16_batch_device": (C.c_int, [C.c_uint16, C.c_uint32, u16p, vpp, u64p, C.c_uint32, u16p, vpp,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vds_ec_repair16_host_batch": (C.c_int, [C.c_uint16, C.c_uint32, u16p, vpp, u64p, C.c_uint32, u16p, vpp,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "vds_ec_base64_decode_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, vpp, u64p, C.c_void_p, C.c_void_p]),
    "vds_ec_base64_encode_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, vpp, C.c_void_p]),
    "vds_ec_upload16_host_batch": (C.c_int, [C.c_uint16, C.c_uint32, C.c_uint32, vpp, u64p, vpp, C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_uint32), vpp, u64p, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_uint32)]),
    "vds_ec_base64_encode_gated_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, vpp, vpp, C.POINTER(C.c_uint32),
                                                          C.c_void_p, C.c_void_p]),
    "vds_ec_download16_batch_device": (C.c_int, [C.c_uint16, C.c_uint32, u16p, vpp, u64p, u16p, C.c_void_p, u16p,
                                                 C.c_void_p, vpp, vpp, vpp, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vds_ec_download16_host_batch": (C.c_int, [C.c_uint16, C.c_uint32, u16p, vpp, u64p, C.c_void_p, u16p,
                                               C.c_void_p, vpp, u64p, C.POINTER(C.c_int32), C.c_void_p,
                                               C.POINTER(C.c_uint32)]),
    "vds_ec_hmac_sha256_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vds_ec_dgram_layout": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, u32p, u32p, u32p]),
    "vds_ec_write_number": (C.c_int, [C.c_uint64, C.c_void_p, u32p]),
    "vds_ec_hmac_sha256_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, u32p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "vds_ec_dgram_seal_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, u32p, vpp, u32p, u32p, C.c_void_p,
                                                 u32p, C.c_uint32, vpp, C.c_uint64, C.c_void_p]),
    "vds_ec_dgram_open_batch_device": (C.c_int, [C.c_uint32, vpp, u32p, u32p, u32p, C.c_void_p, C.c_uint32, vpp,
                                                 C.c_void_p, C.c_void_p]),
    "vds_ec_dgram_seal_host_batch": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, u32p, vpp, u32p, u32p, C.c_void_p,
                                               u32p, C.c_uint32, C.c_void_p, C.c_uint64, u64p, u32p, u32p]),
    "vds_ec_dgram_open_host_batch": (C.c_int, [C.c_uint32, vpp, u32p, u32p, C.c_void_p, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_uint64, C.POINTER(DgramMessage), u32p]),
    "vds_ec_ws_frame_parse": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(WsFrame)]),
    "vds_ec_ws_frame_header": (C.c_int, [C.c_uint64, C.c_int, C.c_void_p, u32p]),
    "vds_ec_ws_upload_request": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, i32p, u64p, u64p, u64p]),
    "vds_ec_ws_upload_answer_size": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, u64p, u32p]),
    "vds_ec_ws_download_answer_layout": (C.c_int, [C.c_int, C.c_uint64, u64p, u32p, u64p]),
    "vds_ec_ws_error_answer": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vds_ec_base64_decode_masked_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, vpp, u64p, C.c_void_p,
                                                           C.c_void_p]),
    "vds_ec_ws_upload_answer_batch_device": (C.c_int, [C.c_uint32, i32p, C.c_uint32, C.c_void_p, C.c_void_p, u32p,
                                                       vpp, C.c_void_p]),
    "vds_ec_ws_upload16_host_batch": (C.c_int, [C.c_uint16, C.c_uint32, C.c_uint32, vpp, u64p, vpp, C.c_void_p,
                                                C.c_void_p, u32p, C.c_void_p, C.c_uint64, u64p, u64p, i32p, u32p]),
    "vds_ec_ws_download16_host_batch": (C.c_int, [C.c_uint16, C.c_uint32, i32p, u16p, vpp, u64p, C.c_void_p, u16p,
                                                  C.c_void_p, C.c_void_p, C.c_uint64, u64p, u64p, i32p, C.c_void_p,
                                                  u32p]),
    "vds_ec_aes256_cbc_padded_size": (C.c_uint64, [C.c_uint64]),
    "vds_ec_block_iv": (C.c_int, [C.c_void_p]),
    "vds_ec_aes256_cbc_encrypt_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vds_ec_aes256_cbc_decrypt_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u64p]),
    "vds_ec_aes256_cbc_encrypt_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p, vpp,
                                                         C.c_void_p]),
    "vds_ec_aes256_cbc_decrypt_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p, vpp,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "vds_ec_block_pack_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, vpp, u64p, C.c_void_p, C.c_void_p, vpp,
                                                 C.c_void_p]),
    "vds_ec_block_pack_host_batch": (C.c_int, [C.c_uint32, vpp, u64p, vpp, u64p, C.c_void_p, C.c_void_p, vpp, u64p]),
    "vds_ec_aes256_cbc_decrypt_host_batch": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p, vpp, u64p,
                                                       i32p, u32p]),
    "vds_ec_inflate_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]),
    "vds_ec_inflate_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, vpp, u64p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vds_ec_inflate_host_batch": (C.c_int, [C.c_uint32, vpp, u64p, vpp, u64p, u64p, i32p, u32p]),
    "vds_ec_deflate_bound": (C.c_uint64, [C.c_uint64]),
    "vds_ec_deflate_host": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]),
    "vds_ec_deflate_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, vpp, u64p, C.c_void_p, C.c_void_p]),
    "vds_ec_deflate_host_batch": (C.c_int, [C.c_uint32, vpp, u64p, vpp, u64p, u64p]),
    "vds_ec_aes256_cbc_encrypt_gated_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p,
                                                               C.c_void_p, vpp, C.c_void_p, C.c_void_p]),
    "vds_ec_block_pack_deflate_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p, vpp, u64p,
                                                         C.c_void_p, C.c_void_p]),
    "vds_ec_block_pack_deflate_host_batch": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p, vpp, u64p,
                                                       u64p]),
    "vds_ec_block_unpack_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p, vpp, u64p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "vds_ec_block_unpack_host_batch": (C.c_int, [C.c_uint32, vpp, u64p, C.c_void_p, C.c_void_p, vpp, u64p, u64p,
                                                 i32p, u32p]),
    "vds_ec_rsa_key_prepare": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(RsaKey)]),
    "vds_ec_rsa_fingerprint": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vds_ec_rsa_public_host": (C.c_int, [C.POINTER(RsaKey), C.c_void_p, C.c_uint64, C.c_void_p]),
    "vds_ec_rsa_verify_sha256_host": (C.c_int, [C.POINTER(RsaKey), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                C.c_void_p]),
    "vds_ec_rsa_public_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, u32p, C.POINTER(RsaKey), C.c_uint32, vpp,
                                                 C.c_void_p, C.c_void_p]),
    "vds_ec_rsa_verify_digest_batch_device": (C.c_int, [C.c_uint32, C.c_void_p, vpp, u64p, u32p, C.POINTER(RsaKey),
                                                        C.c_uint32, C.c_void_p, C.c_void_p]),
    "vds_ec_rsa_verify_sha256_batch_device": (C.c_int, [C.c_uint32, vpp, u64p, vpp, u64p, u32p, C.POINTER(RsaKey),
                                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vds_ec_txblock_parse": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(TxBlock)]),
    "vds_ec_txblock_validate_host_batch": (C.c_int, [C.c_uint32, vpp, u64p, C.POINTER(RsaKey), C.c_void_p, C.c_uint32,
                                                     C.c_void_p, C.c_void_p, i32p]),
    "vds_ec_base64_decoded_size": (C.c_size_t, [C.c_char_p, C.c_size_t]),
    "vds_ec_base64_decode": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]),
    "vds_ec_base64_encode": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vds_ec_tmp_names": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "vds_ec_upload_response_json": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                              C.c_size_t, C.POINTER(C.c_size_t)]),
    "vds_ec_save_temp16_host": (C.c_int, [C.c_uint16, C.c_uint32, C.c_void_p, C.c_uint64, vpp, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_uint32)]),
    "vds_ec_encode16_range_device": (C.c_int, [C.c_uint16, u16p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                                               C.c_uint64, vpp, C.c_uint, C.c_void_p]),
    "vds_ec_restore16_range_device": (C.c_int, [C.c_uint16, u16p, vpp, C.c_uint64, C.c_uint16, C.c_uint64,
                                                C.c_uint64, C.c_void_p, C.c_uint, C.c_void_p]),
    "vds_ec_encode16_host_split": (C.c_int, [C.c_uint16, u16p, C.c_uint32, C.c_void_p, C.c_uint64, vpp, C.c_uint,
                                             C.c_int, C.c_uint32]),
    "vds_ec_restore16_host_split": (C.c_int, [C.c_uint16, u16p, vpp, C.c_uint64, C.c_void_p, u64p, C.c_uint, C.c_int,
                                              C.c_uint32]),
}

_lib = None
_lock = threading.Lock()


class VdsEcError(RuntimeError):
    """A non-zero vds_ec status (the C++ drop-in maps these to
    make_unexpected<std::runtime_error>, expected.h:46-49)."""

    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = strerror(status)
        super().__init__(f"{what}: {msg}" if what else msg)


def _bind_runtime_first() -> None:
    """Load torch's HIP runtime before ours when torch is installed.

    torch ships its own libamdhip64.so (soname libamdhip64.so.7) and links it
    under the unversioned name; if libvds_ec.so (NEEDED libamdhip64.so.7 from
    /opt/rocm) were loaded first, importing torch afterwards would map a second
    HIP runtime into the process.  Loading torch first makes our NEEDED entry
    resolve to the runtime already present, so there is exactly one.
    """
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                _bind_runtime_first()
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(f"{LIB_PATH} is missing: run vds_amd/build.py (no CPU fallback)")
                h = C.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    f = getattr(h, name)
                    f.restype = res
                    f.argtypes = args
                _lib = h
    return _lib


def strerror(status: int) -> str:
    try:
        return lib().vds_ec_strerror(status).decode()
    except Exception:  # pragma: no cover - library unavailable
        return f"vds_ec status {status}"


def check(status: int, what: str = "") -> None:
    if status != OK:
        raise VdsEcError(status, what)


def device_count() -> int:
    n = C.c_int(0)
    check(lib().vds_ec_device_count(C.byref(n)))
    return n.value
