"""The C-ABI boundary of the RSA verification, no GPU: the entry points exist
under their C names, the new status codes have texts of their own, the version
is bumped, the structures have the layout the bindings assume, and the device
forms validate before they look for a device."""
import ctypes as C
import os
import re
import subprocess

import rsa_cases as R
from vds_amd import _lib, chunk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vds_ec_rsa_key_prepare", "vds_ec_rsa_fingerprint", "vds_ec_rsa_public_host", "vds_ec_rsa_verify_sha256_host",
         "vds_ec_rsa_public_batch_device", "vds_ec_rsa_verify_digest_batch_device",
         "vds_ec_rsa_verify_sha256_batch_device", "vds_ec_txblock_parse", "vds_ec_txblock_validate_host_batch")


def test_symbols_have_c_names(vds_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vds_amd", "libvds_ec.so")],
                        capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(vds_ec_\w+)\b", nm))
    for name in NAMES:
        assert name in exported and name in _lib.SIGNATURES and hasattr(vds_lib, name), name


def test_status_codes_and_version(vds_lib):
    assert (_lib.ETX_FORM, _lib.ETX_KEY) == (-23, -24)
    texts = {s: vds_lib.vds_ec_strerror(s) for s in range(-24, 1)}
    assert len(set(texts.values())) == 25
    assert b"unknown" not in texts[-23] and b"unknown" not in texts[-24]
    assert b"unknown" in vds_lib.vds_ec_strerror(-25)
    assert vds_lib.vds_ec_version() >= 103


def test_structures_are_fixed_size_pods():
    assert C.sizeof(_lib.RsaKey) == 2 * 4 * 128 + 16
    assert C.sizeof(_lib.TxBlock) == 12 * 8
    header = open(os.path.join(ROOT, "include", "vds_ec.h")).read()
    assert "#define VDS_EC_RSA_MAX_LIMBS 128" in header


def test_device_forms_validate_before_the_device(vds_lib):
    """count == 0 is OK and null arrays with count > 0 are VDS_EC_EINVAL, with or without a GPU."""
    key = chunk.rsa_key_prepare(R.kats()["keys"][2]["n"], 65537)
    keys = (_lib.RsaKey * 1)(key)
    one = (C.c_void_p * 1)(64)
    ln = (C.c_uint64 * 1)(256)
    ki = (C.c_uint32 * 1)(0)
    dev = C.c_void_p(64)  # never dereferenced: every call below ends in validation
    assert vds_lib.vds_ec_rsa_public_batch_device(0, None, None, None, None, 0, None, None, None) == 0
    assert vds_lib.vds_ec_rsa_verify_digest_batch_device(0, None, None, None, None, None, 0, None, None) == 0
    assert vds_lib.vds_ec_rsa_verify_sha256_batch_device(0, None, None, None, None, None, None, 0, None, None, None) == 0
    assert vds_lib.vds_ec_txblock_validate_host_batch(0, None, None, None, None, 0, None, None, None) == 0
    E = _lib.EINVAL
    assert vds_lib.vds_ec_rsa_public_batch_device(1, None, ln, ki, keys, 1, one, dev, None) == E
    assert vds_lib.vds_ec_rsa_public_batch_device(1, one, None, ki, keys, 1, one, dev, None) == E
    assert vds_lib.vds_ec_rsa_public_batch_device(1, one, ln, None, keys, 1, one, dev, None) == E
    assert vds_lib.vds_ec_rsa_public_batch_device(1, one, ln, ki, None, 1, one, dev, None) == E
    assert vds_lib.vds_ec_rsa_public_batch_device(1, one, ln, ki, keys, 1, None, dev, None) == E
    assert vds_lib.vds_ec_rsa_public_batch_device(1, one, ln, ki, keys, 1, one, None, None) == E
    assert vds_lib.vds_ec_rsa_public_batch_device(1 << 30, one, ln, ki, keys, 1, one, dev, None) == E
    ki[0] = 1  # key_idx[o] >= nkeys
    assert vds_lib.vds_ec_rsa_public_batch_device(1, one, ln, ki, keys, 1, one, dev, None) == E
    assert vds_lib.vds_ec_rsa_verify_digest_batch_device(1, dev, one, ln, ki, keys, 1, dev, None) == E
    assert vds_lib.vds_ec_rsa_verify_sha256_batch_device(1, one, ln, one, ln, ki, keys, 1, dev, None, None) == E
    ki[0] = 0
    assert vds_lib.vds_ec_rsa_verify_digest_batch_device(1, None, one, ln, ki, keys, 1, dev, None) == E
    assert vds_lib.vds_ec_rsa_verify_digest_batch_device(1, dev, one, ln, ki, keys, 1, None, None) == E
    assert vds_lib.vds_ec_rsa_verify_sha256_batch_device(1, None, ln, one, ln, ki, keys, 1, dev, None, None) == E
    keys[0].limbs = 65  # a key that vds_ec_rsa_key_prepare did not make
    assert vds_lib.vds_ec_rsa_verify_digest_batch_device(1, dev, one, ln, ki, keys, 1, dev, None) == E
    assert vds_lib.vds_ec_txblock_validate_host_batch(1, one, ln, keys, dev, 1, dev, dev, None) == E
