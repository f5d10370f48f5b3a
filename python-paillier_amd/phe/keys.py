"""Key objects of the drop-in: same constructor signatures, attributes, equality/hash and error
behaviour as the reference (phe/paillier.py:37-68 keypair generation, :71-194 PaillierPublicKey,
:197-380 PaillierPrivateKey, :383-439 PaillierPrivateKeyring), with the arithmetic delegated to a
per-key GPU Engine and batched siblings (`*_batch`) added next to every scalar method.

Key generation and the once-per-key constants (p_inverse, hp, hq) are cold, host-side integer work
(out of the hot path); everything per-ciphertext runs on the GPU.
"""
import math
import random
import threading

try:
    from collections.abc import Mapping
except ImportError:  # pragma: no cover
    Mapping = dict

import numpy as np

from . import util
from . import _engine
from ._engine import Engine, random_lt_n, random_lt_n_limbs
from .codec import EncodedNumber
from .sharding import shard_bounds

DEFAULT_KEYSIZE = 3072
# scalar encrypt() / obfuscate() refill the obfuscator pool with this many r^n per launch when it runs dry (0 = one
# exponentiation per call, as the reference does): 4096 rows still fit the latency geometry of one launch
SCALAR_POOL_REFILL = 4096
# decrypt_packed returning a LIST also goes through the unpack kernel where it can (False: lists are unpacked on the host, only
# as_array=True takes the kernel)
PACKED_LISTS_THROUGH_CODEC = True
# encrypt_batch forms the plaintext rows of int64 / uint64 / float64 arrays on the GPU (Engine.values_encode_dev) from this many
# values on; below it the host encoding stays (same bits either way).  The crossover is measured by tools/bench_value_codec.py
# (profiles/r15_value_codec.json)
VALUE_CODEC_DEVICE_MIN = 2048


def _gpu_prime_search_available():
    """the batched Miller-Rabin launch needs the real library and a device (the test emulator has neither)"""
    try:
        from . import _native
        return hasattr(_native.Context, "encrypt_dev") and _native.device_count() > 0
    except Exception:
        return False


def generate_paillier_keypair(private_keyring=None, n_length=DEFAULT_KEYSIZE):
    """New (PaillierPublicKey, PaillierPrivateKey) with an n of exactly n_length bits (phe/paillier.py:37-68)."""
    half = n_length // 2
    draw_pair = None
    if half >= 256 and _gpu_prime_search_available():
        # both primes of a try from ONE pair of launches (phe/primes.py: the smallest probable prime above a random
        # start with the top bit set — the gmpy2 branch of getprimeover, phe/util.py:113-116)
        from . import primes
        draw_pair = lambda: primes.getprimeover_batch(half, 2)
    while True:
        if draw_pair is not None:
            p, q = draw_pair()
            if p == q:
                continue
        else:
            p = util.getprimeover(half)
            q = p
            while q == p:
                q = util.getprimeover(half)
        n = p * q
        if n.bit_length() == n_length:
            break
    public_key = PaillierPublicKey(n)
    private_key = PaillierPrivateKey(public_key, p, q)
    if private_keyring is not None:
        private_keyring.add(private_key)
    return public_key, private_key


class PaillierPublicKey(object):
    def __init__(self, n):
        self.g = n + 1
        self.n = n
        self.nsquare = n * n
        self.max_int = n // 3 - 1
        self._engine = None
        self._engine_lock = threading.Lock()
        self._fleet = None
        self._fleet_factory = None               # device -> Engine for the further devices of a fleet (a key pair installs its own)
        self._short = None                       # (h_s, bits) while short-exponent obfuscators are on (enable_short_obfuscators)
        self._short_rng = False                  # its device_rng flag: rho of whole batches from per-launch ChaCha20 seeds

    # one GPU context per key, created on first use (a private key shares its context with its public key); the creation
    # is guarded so that two threads never build two contexts — and two obfuscator pools — for one key
    def _get_engine(self):
        eng = self._engine
        if eng is None:
            with self._engine_lock:
                if self._engine is None:
                    self._engine = Engine(self.n)
                eng = self._engine
        return self._short_sync(eng)

    def _short_sync(self, eng):
        """the engine, told the key's short-obfuscator setting if it does not have it yet (every engine of the key — of a fleet,
        or one that took over from another — builds its own table from it, on first use)"""
        want = self._short
        if eng.short_base() != want:
            eng.set_short_base(*(want or (None, 0)))
        if eng.short_device_rng() != self._short_rng:
            eng.set_short_device_rng(self._short_rng)
        return eng

    def _get_fleet(self):
        """One engine per device of PHE_HIP_DEVICES (phe/fleet.py), the key's ordinary engine first — or None when no
        single-process fan-out is asked for.  A key pair shares one fleet, as it shares one engine."""
        fl = self._fleet
        if fl is not None:
            return fl
        from . import fleet
        devices = fleet.configured_devices()
        if devices is None:
            return None
        primary = self._get_engine()
        with self._engine_lock:
            if self._fleet is None or self._fleet.engine(0) is not self._engine:
                make = self._fleet_factory or (lambda device: Engine(self.n, device=device))
                self._fleet = fleet.Fleet(self._engine or primary, make, devices)
            return self._fleet

    def _engine_for(self, store):
        """the engine that owns a resident array (a vector made by encrypt_batch_sharded lives on ITS device), else the
        key's ordinary engine"""
        primary = self._get_engine()
        ctx = getattr(store, "ctx", None)
        if ctx is None or ctx is primary.ctx:
            return primary
        fl = self._fleet
        if fl is not None:
            eng = fl.engine_of(ctx)
            if eng is not None:
                return self._short_sync(eng)
        device = getattr(ctx, "device", None)
        if device is None or device == primary.device:
            return primary          # another context of the primary's GPU (e.g. the public engine a key pair's engine replaced)
        if fl is not None:
            eng = fl.engine_on(device)
            if eng is not None:
                return self._short_sync(eng)
        # never launch one device's kernels on another device's pointers (nothing here enables peer access)
        raise RuntimeError("resident rows live on device %r, which no engine of this key serves (engines on %r): move them "
                           "through the host (vector.to_host())" % (device, [primary.device] + (fl.devices[1:] if fl else [])))

    def __repr__(self):
        return "<PaillierPublicKey {}>".format(hex(hash(self))[2:][:10])

    def __eq__(self, other):
        return self.n == other.n

    def __hash__(self):
        return hash(self.n)

    def __getstate__(self):  # engines hold device handles; keys pickle as plain numbers
        return {"n": self.n}

    def __setstate__(self, state):
        self.__init__(state["n"])

    def get_random_lt_n(self):
        return random.SystemRandom().randrange(1, self.n)

    # ---- scalar API (batch of one on the GPU) ---------------------------------------------------
    def raw_encrypt(self, plaintext, r_value=None):
        if not isinstance(plaintext, int):
            raise TypeError('Expected int type plaintext but got: %s' % type(plaintext))
        r = r_value or self.get_random_lt_n()          # falsy r_value (None, 0) => random, as in the reference
        return self.raw_encrypt_batch([plaintext], [r])[0]

    def encrypt(self, value, precision=None, r_value=None):
        encoding = value if isinstance(value, EncodedNumber) else EncodedNumber.encode(self, value, precision)
        return self.encrypt_encoded(encoding, r_value)

    def encrypt_encoded(self, encoding, r_value):
        from .ciphertext import EncryptedNumber
        if r_value is None:
            # fresh obfuscator: one fused launch (1 + n*m) * r^n, flagged obfuscated like
            # encrypt_encoded + obfuscate() in the reference (phe/paillier.py:189-193)
            eng = self._get_engine()
            if hasattr(eng.ctx, "encrypt_dev"):
                # an obfuscator r^n made ahead of time (precompute_obfuscators), used once: r^n * (1 + n m), one small
                # launch.  One scalar encryption is one latency-bound exponentiation on an otherwise idle GPU: when the
                # pool is dry, draw and exponentiate a launch-full of obfuscators in the same ~time and keep the rest
                if not isinstance(encoding.encoding, int):
                    raise TypeError('Expected int type plaintext but got: %s' % type(encoding.encoding))
                plain = eng.plain_limbs([encoding.encoding % self.n])
                limbs = eng.encrypt_from_obfuscators(plain)
                if limbs is None and SCALAR_POOL_REFILL:
                    eng.fill_obfuscator_pool(SCALAR_POOL_REFILL)
                    limbs = eng.encrypt_from_obfuscators(plain)
                if limbs is not None:
                    number = EncryptedNumber(self, eng.to_ints(limbs.to_host())[0], encoding.exponent)
                    number._EncryptedNumber__is_obfuscated = True
                    return number
            if self._short is not None:
                if not isinstance(encoding.encoding, int):
                    raise TypeError('Expected int type plaintext but got: %s' % type(encoding.encoding))
                c = eng.to_ints(eng.short_pow(self._draw_rho(eng, 1), m=[encoding.encoding]))[0]
            else:
                c = self.raw_encrypt(encoding.encoding, self.get_random_lt_n())
            number = EncryptedNumber(self, c, encoding.exponent)
            number._EncryptedNumber__is_obfuscated = True
            return number
        c = self.raw_encrypt(encoding.encoding, r_value or 1)   # r_value == 0 => obfuscator 1, not obfuscated
        return EncryptedNumber(self, c, encoding.exponent)

    # ---- offline / online split ------------------------------------------------------------------------
    def precompute_obfuscators(self, count, sharded=False):
        """Make `count` obfuscators r^n mod n^2 (fresh r from the OS CSPRNG) ahead of time and keep them in HBM.
        encrypt_batch without r_values and EncryptedVector.obfuscate() then consume them — one product per element
        instead of a modular exponentiation — and fall back to drawing on the spot when the pool is short.  Every
        obfuscator is used once.  Returns the number available.  With a fleet (PHE_HIP_DEVICES) the pool is cut the way the
        batch that will consume it is cut: `encrypt_batch` of `count` rows by default, `encrypt_batch_sharded` of `count` rows
        (one part per device whatever the size) with sharded=True."""
        fl = self._get_fleet()
        count = int(count)
        bounds = fl.shards(count, min_rows=1 if sharded else None) if fl is not None else []
        if len(bounds) > 1:
            # the devices a batch of `count` rows fans out to fill THEIR pools with the shares that batch will take from them
            # (a pool is never shared across devices; a batch too small to fan out, and every scalar call, is served by the
            # primary engine alone — so a small `count` goes there whole instead of being spread where nothing would use it)
            futures = [fl._pool.submit(self._short_sync(fl.engine(k)).fill_obfuscator_pool, hi - lo)
                       for k, (lo, hi) in enumerate(bounds)]
            for f in futures:
                f.result()
            return self.obfuscators_available()
        return self._get_engine().fill_obfuscator_pool(count)

    def obfuscators_available(self, per_device=False):
        """obfuscators made ahead of time and not used yet; per_device=True: the list, one entry per engine that exists (an
        obfuscator is only ever used by the device that holds it)"""
        fl = self._fleet
        counts = [eng.obfuscators_available() for eng in (fl.made() if fl is not None else [self._get_engine()])]
        return counts if per_device else sum(counts)

    def discard_obfuscators(self):
        """forget the obfuscators made ahead of time: the next encryptions draw and exponentiate on the spot again"""
        fl = self._fleet
        for eng in (fl.made() if fl is not None else [self._get_engine()]):
            eng.clear_obfuscator_pool()

    # ---- short-exponent obfuscators ---------------------------------------------------------------------
    def enable_short_obfuscators(self, bits=None, x=None, hs=None, device_rng=False):
        """Draw every fresh obfuscator as h_s^rho mod n^2 for a short random exponent rho in [0, 2^bits) instead of r^n for a
        fresh r in [1, n) — the variant of Damgard, Jurik and Nielsen that production Paillier stacks offer.  With a
        unit x, h = -x^2 mod n and h_s = h^n mod n^2, the obfuscator h_s^rho = (h^rho)^n is an n-th power, so decryption is
        unchanged, and c = (1 + n m) * h_s^rho is bit for bit raw_encrypt(m, r_value=pow(h, rho, n)).  The base is the same for
        every ciphertext: the GPU multiplies ceil(bits / w) entries of a table of powers of h_s and squares nothing
        (csrc/fixed_base.h).  Returns h_s.
        bits: the length of rho, default n.bit_length() // 2 (outside [1, n.bit_length()]: ValueError; not an integer:
        TypeError).  x: the unit h is made of, default a CSPRNG draw from [1, n) with gcd(x, n) = 1 (a given x that shares a
        factor with n, or lies outside [1, n): ValueError).  hs: a ready h_s handed out by the key owner, instead of x (both:
        ValueError); it must satisfy 1 < hs < n^2 and be coprime to n.
        AN h_s THAT IS NOT AN n-TH POWER CORRUPTS EVERY PLAINTEXT ENCRYPTED WITH IT, AND NOTHING HERE CAN DETECT THAT: a public
        key cannot tell n-th powers from other residues — that is the assumption Paillier encryption rests on.  Take hs only
        from whoever made the key.
        What the scheme assumes beyond the reference's: that h_s^rho for short rho cannot be told from a random n-th power
        (short exponents in the subgroup generated by h).  It applies from now on to encrypt, encrypt_batch, encrypt_packed,
        encrypt_batch_sharded, precompute_obfuscators and obfuscate(); explicit r_values keep meaning the reference's r, and
        obfuscators already in the pool stay valid and are used up.  The setting is not part of ==, hash() or pickling.
        device_rng (off by default): where the exponents of a whole batch come from.  Off: every rho is read from the kernel
        CSPRNG (/dev/urandom) by the host and uploaded.  On: for encrypt_batch, encrypt_packed, encrypt_batch_sharded,
        precompute_obfuscators and whole-vector obfuscate(), the host reads only a 32-byte seed per launch from the kernel CSPRNG
        and the rho are the ChaCha20 keystream (RFC 8439, 20 rounds) under that 256-bit key, expanded on the GPU where the comb
        kernel reads them — the construction /dev/urandom itself uses, one level down.  A seed is used for one launch, travels
        in the kernel's arguments, is overwritten on the host when the launch call returns and is never cached, logged or put in
        an error message; it is as sensitive as the exponents it expands to.  Scalar calls and obfuscate(rows=...) keep the host
        draw; rho_values= and r_values= are unaffected."""
        nbits = self.n.bit_length()
        if bits is None:
            bits = nbits // 2
        if isinstance(bits, (bool, np.bool_)) or not isinstance(bits, (int, np.integer)):
            raise TypeError("bits must be an integer")
        bits = int(bits)
        if not 1 <= bits <= nbits:
            raise ValueError("bits must lie in [1, %d]" % nbits)
        if x is not None and hs is not None:
            raise ValueError("give x or hs, not both")
        if hs is None:
            if x is None:
                rng = random.SystemRandom()
                x = rng.randrange(1, self.n)
                while math.gcd(x, self.n) != 1:
                    x = rng.randrange(1, self.n)
            else:
                if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                    raise TypeError("x must be an integer")
                x = int(x)
                if not 1 <= x < self.n or math.gcd(x, self.n) != 1:
                    raise ValueError("x must lie in [1, n) and share no factor with n")
            hs = pow((-x * x) % self.n, self.n, self.nsquare)
        else:
            if isinstance(hs, (bool, np.bool_)) or not isinstance(hs, (int, np.integer)):
                raise TypeError("hs must be an integer")
            hs = int(hs)
        if not 1 < hs < self.nsquare or math.gcd(hs, self.n) != 1:
            raise ValueError("h_s must lie in (1, n^2) and share no factor with n")
        self._short = (hs, bits)
        self._short_rng = bool(device_rng)
        return hs

    def disable_short_obfuscators(self):
        """fresh obfuscators are r^n for r in [1, n) again (the reference's); the tables of powers of h_s are dropped"""
        self._short = None
        self._short_rng = False
        fl = self._fleet
        for eng in (fl.made() if fl is not None else [self._engine] if self._engine is not None else []):
            self._short_sync(eng)

    @property
    def short_obfuscator_base(self):
        """h_s while short-exponent obfuscators are on, else None"""
        return self._short[0] if self._short is not None else None

    @property
    def short_obfuscator_bits(self):
        """the length of the exponents rho while short-exponent obfuscators are on, else None"""
        return self._short[1] if self._short is not None else None

    @property
    def short_obfuscator_device_rng(self):
        """True while the exponents of whole batches are ChaCha20 output under per-launch seeds (enable_short_obfuscators
        (device_rng=True)), else False"""
        return self._short is not None and self._short_rng

    def _draw_rho(self, eng, count):
        """`count` fresh exponents as limb rows: from the kernel CSPRNG — or, for more than one row under the device_rng
        setting, expanded from a fresh seed on the host (a lone row is 128 bytes: read directly)"""
        bits = self._short[1]
        if self._short_rng and count > 1:
            return _engine.seeded_bits_limbs(bits, count, (bits + 31) // 32)
        return _engine.random_bits_limbs(bits, count, (bits + 31) // 32)

    def _rho_limbs(self, rho_values, count, r_values=None):
        """the explicit exponents of a `rho_values=` argument as (count, ceil(bits / 32)) limb rows, checked"""
        from . import _native
        if r_values is not None:
            raise ValueError("give r_values or rho_values, not both")
        if self._short is None:
            raise ValueError("rho_values need short obfuscators: call enable_short_obfuscators() first")
        bits = self._short[1]
        el = (bits + 31) // 32
        if isinstance(rho_values, np.ndarray) and rho_values.ndim == 2:
            if rho_values.dtype != np.uint32 or rho_values.shape != (count, el):
                raise ValueError("rho_values as an array must be (%d, %d) uint32 rows, not %s %s"
                                 % (count, el, rho_values.shape, rho_values.dtype))
            if bits < 32 * el:
                bad = np.flatnonzero(rho_values[:, el - 1] >> np.uint32(bits - 32 * (el - 1)))
                if len(bad):
                    raise ValueError("rho_values[%d] lies outside [0, 2^%d)" % (bad[0], bits))
            return np.ascontiguousarray(rho_values)
        vals = [int(v) if isinstance(v, np.integer) else v for v in rho_values]
        if len(vals) != count:
            raise ValueError("%d rho_values for %d rows" % (len(vals), count))
        for i, v in enumerate(vals):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError("rho_values[%d] is not an integer" % i)
            if not 0 <= v < 1 << bits:
                raise ValueError("rho_values[%d] lies outside [0, 2^%d)" % (i, bits))
        return _native.ints_to_limbs(vals, el)

    # ---- batched API ------------------------------------------------------------------------------
    def raw_encrypt_batch(self, plaintexts, r_values=None):
        """List of ints -> list of int ciphertexts; r_values=None draws fresh obfuscators."""
        plaintexts = list(plaintexts)
        for m in plaintexts:
            if not isinstance(m, int):
                raise TypeError('Expected int type plaintext but got: %s' % type(m))
        if r_values is None:
            r_values = random_lt_n(self.n, len(plaintexts))
        eng = self._get_engine()
        return eng.to_ints(eng.raw_encrypt(plaintexts, list(r_values)))

    def encrypt_batch(self, values, precision=None, r_values=None, device=False, rho_values=None):
        """Encode + encrypt a whole sequence / numpy array -> EncryptedVector (one kernel launch).
        device=True keeps the ciphertexts resident in HBM for later homomorphic operations.
        float64 / integer numpy arrays are encoded and drawn without a Python integer per element; from
        VALUE_CODEC_DEVICE_MIN values on, int64 / uint64 / float64 arrays (float64 also under a `precision`: one common
        exponent, mantissas rounded half to even) are encoded on the GPU and only their 8 bytes per value are uploaded
        (Engine.values_encode_dev: same bits, exponents and exceptions as the host encoding).
        rho_values (with enable_short_obfuscators): the exponents of the obfuscators h_s^rho given explicitly, as integers in
        [0, 2^bits) or (count, ceil(bits / 32)) uint32 rows — row i is raw_encrypt(m_i, r_value=pow(h, rho_i, n))."""
        from .ciphertext import EncryptedVector
        from ._device import DeviceArray
        eng = self._get_engine()
        fresh = r_values is None and rho_values is None
        m = exps = None
        arr = self._value_codec_array(eng, values, precision, device)
        if arr is not None:
            # the rows are formed where they are used (Engine.values_encode_dev): 8 bytes per value go up, the exponents and a
            # status byte come down; this happens — and raises — before any pool obfuscator is taken
            if precision is None:
                got = eng.values_encode_dev(arr)
            else:
                try:
                    got = eng.values_encode_dev(arr, EncodedNumber._natural_exponent(0.0, precision))
                except ValueError:
                    got = None                                     # inf / nan under a precision: the host route's own exceptions
            if got is not None:
                m, exps = got
                if precision is not None:
                    exps = np.full(len(arr), exps, dtype=np.int64)
        if m is None:
            signed = EncodedNumber.encode_signed(values, precision) if eng.n_limbs >= 4 else None
            if signed is not None:
                mag, neg, exps = signed
                m = EncodedNumber.signed_to_limbs(self, mag, neg, eng.n_limbs)
            else:
                m, exps = EncodedNumber.encode_many(self, values, precision)
        resident = isinstance(m, DeviceArray)
        count = len(exps)
        limbs = None
        if rho_values is not None:
            rho = self._rho_limbs(rho_values, count, r_values)
            if resident:
                limbs = eng.short_pow_dev(rho, m=m)
                limbs = limbs if device else limbs.to_host()
            else:
                limbs = eng.short_pow_dev(rho, m=m) if device else eng.short_pow(rho, m=m)
            return EncryptedVector(self, limbs, exps, obfuscated=False)
        fl = self._get_fleet() if (not device and isinstance(m, np.ndarray)) else None
        if fl is not None and len(fl.shards(count)) > 1:
            # single-process fan-out (phe/fleet.py): contiguous shards, one device each, results into ONE host array
            if fresh:
                def shard(e, lo, hi):
                    self._short_sync(e)
                    if not hasattr(e.ctx, "encrypt_dev"):           # (a backend without resident rows: draw, then one call)
                        if self._short is not None:
                            return e.short_pow(self._draw_rho(e, hi - lo), m=m[lo:hi])
                        return e.raw_encrypt(m[lo:hi], random_lt_n_limbs(self.n, hi - lo, e.n_limbs))
                    got = e.encrypt_from_obfuscators(m[lo:hi])      # the device's own pool first (each obfuscator used once)
                    return got.to_host() if got is not None else e.raw_encrypt_fresh(m[lo:hi], False)
            else:
                r_all = r_values if isinstance(r_values, np.ndarray) else eng.plain_limbs(list(r_values))
                shard = lambda e, lo, hi: e.raw_encrypt(m[lo:hi], r_all[lo:hi])
            return EncryptedVector(self, np.concatenate(fl.run(count, shard)), exps, obfuscated=fresh)
        if fresh and isinstance(m, (np.ndarray, DeviceArray)) and hasattr(eng.ctx, "encrypt_dev"):
            # online part only: (1 + n m) * r^n with r^n from the pool made by precompute_obfuscators (each used once)
            limbs = eng.encrypt_from_obfuscators(m)
            if limbs is None and 0 < count <= SCALAR_POOL_REFILL // 4:
                eng.fill_obfuscator_pool(SCALAR_POOL_REFILL)       # a small batch is as latency-bound as a scalar call
                limbs = eng.encrypt_from_obfuscators(m)
        if limbs is not None:
            if not device:
                limbs = limbs.to_host()
        elif fresh and isinstance(m, (np.ndarray, DeviceArray)) and hasattr(eng.ctx, "encrypt_dev"):
            limbs = eng.raw_encrypt_fresh(m, device)
        elif fresh and self._short is not None and not resident:
            rho = self._draw_rho(eng, count)
            limbs = eng.short_pow_dev(rho, m=m) if device else eng.short_pow(rho, m=m)
        else:
            r = random_lt_n_limbs(self.n, count, eng.n_limbs) if fresh else list(r_values)
            if resident and not device:
                if len(r) != count:
                    raise ValueError("m and r batch sizes differ")
                limbs = eng.raw_encrypt_dev(m, r).to_host()        # resident rows in, the ciphertexts come down
            else:
                limbs = eng.raw_encrypt_dev(m, r) if device else eng.raw_encrypt(m, r)
        return EncryptedVector(self, limbs, exps, obfuscated=fresh)

    def _value_codec_array(self, eng, values, precision, device):
        """the array encrypt_batch hands to the device codec (Engine.values_encode_dev) — int64, uint64 or float64, flat — or
        None where the host encoding stays: other element types (lists become arrays by the rules of
        EncodedNumber.encode_signed), integers with a precision, another BASE than 16, a key with max_int < 2^64, a backend
        without the kernels, a batch below VALUE_CODEC_DEVICE_MIN, or a host batch that the fleet fans out."""
        if EncodedNumber.BASE != 16 or EncodedNumber.FLOAT_MANTISSA_BITS != 53 or not eng.has_value_codec():
            return None
        if isinstance(values, (list, tuple)) and len(values) >= max(1, VALUE_CODEC_DEVICE_MIN):
            kind = type(values[0])
            if kind is float and all(type(v) is float for v in values):
                values = np.array(values, dtype=np.float64)
            elif kind is int and precision is None and all(type(v) is int for v in values):
                try:
                    values = np.array(values, dtype=np.int64)
                except OverflowError:
                    return None
        if not isinstance(values, np.ndarray) or values.size < max(1, VALUE_CODEC_DEVICE_MIN):
            return None
        if values.dtype == np.float64:
            arr = values.reshape(-1)
        elif values.dtype.kind in "iu" and precision is None:
            arr = values.reshape(-1).astype(np.uint64 if values.dtype.kind == "u" else np.int64, copy=False)
        else:
            return None
        if not device:
            fl = self._get_fleet()
            if fl is not None and len(fl.shards(len(arr))) > 1:
                return None
        return arr

    def _packed_mantissas(self, values, precision):
        """(signed mantissas, exponent) of encrypt_packed: element-wise the int_rep and exponent that
        EncodedNumber.encode(self, v, precision=precision) picks, all at ONE exponent (ValueError otherwise).  The mantissas come
        back as an int64 array where numpy can make them — int arrays, float64 arrays, homogeneous lists of either — and as a
        list of Python integers otherwise."""
        if isinstance(values, (list, tuple)) and len(values):
            kind = type(values[0])
            if kind is float and all(type(v) is float for v in values):
                values = np.array(values, dtype=np.float64)
            elif kind is int and all(type(v) is int for v in values):
                try:
                    values = np.array(values, dtype=np.int64)
                except OverflowError:
                    pass
        log2b = int(round(EncodedNumber.LOG2_BASE))
        pow2_base = (1 << log2b) == EncodedNumber.BASE
        if isinstance(values, np.ndarray):
            arr = values.reshape(-1)
            if arr.dtype.kind in "iu" and precision is None and (arr.dtype.kind == "i" or arr.dtype.itemsize < 8):
                return arr.astype(np.int64), 0
            if arr.dtype == np.float64 and pow2_base and len(arr):
                if not np.all(np.isfinite(arr)):
                    raise ValueError("cannot encode inf / nan")
                if precision is not None:
                    # one exponent for all; BASE^-exponent is a power of two, so the scaling is exact and np.rint rounds
                    # the exact quotient half to even, as round(Fraction) does
                    exponent = EncodedNumber._natural_exponent(0.0, precision)
                    scaled = np.ldexp(arr, -exponent * log2b)
                    if np.all(np.abs(scaled) < 2.0 ** 62):             # (beyond that — or inf —: element by element)
                        return np.rint(scaled).astype(np.int64), exponent
                elif log2b + EncodedNumber.FLOAT_MANTISSA_BITS <= 62:
                    mag, neg, exps = EncodedNumber.encode_signed(arr)
                    differ = np.flatnonzero(exps != exps[0])
                    if len(differ):
                        raise ValueError("the value at index %d encodes at exponent %d, the first at %d: give a precision"
                                         % (differ[0], exps[differ[0]], exps[0]))
                    rep = mag.astype(np.int64)
                    np.negative(rep, out=rep, where=neg)
                    return rep, int(exps[0])
            values = arr.tolist()
        reps, exponent = [], None
        n, max_int = self.n, self.max_int
        for i, v in enumerate(values):
            e = EncodedNumber.encode(self, v, precision=precision)
            if exponent is None:
                exponent = e.exponent
            elif e.exponent != exponent:
                raise ValueError("the value at index %d encodes at exponent %d, the first at %d: give a precision"
                                 % (i, e.exponent, exponent))
            reps.append(e.encoding if e.encoding <= max_int else e.encoding - n)
        return reps, (0 if exponent is None else exponent)

    def _pack_plain_host(self, mantissas, slots, slot_bits):
        """the packed plaintext rows of encrypt_packed on the host: row b = (sum_j x[b*S + j] * 2^(B j)) mod n as limb rows.
        With u = sum_j (x_j + 2^(B-1)) 2^(B j) — B-bit fields, placed by numpy for B <= 64 — the row is (u - offset) mod n:
        one Python integer per ROW."""
        from . import _native
        S, B, n = slots, slot_bits, self.n
        count = len(mantissas)
        rows = -(-count // S)
        n_limbs = self._get_engine().n_limbs
        if isinstance(mantissas, np.ndarray) and B <= 64:
            half = 1 << (B - 1)
            x = np.zeros(rows * S, dtype=np.int64)
            x[:count] = mantissas
            fields = (x.view(np.uint64) + np.uint64(half)) & np.uint64((1 << B) - 1)      # (wraps for B = 64: x ^ 2^63)
            fields = fields.reshape(rows, S)
            n_words = (S * B + 63) // 64 + 1
            words = np.zeros((rows, n_words), dtype=np.uint64)
            for j in range(S):
                w, off = divmod(B * j, 64)
                words[:, w] |= fields[:, j] << np.uint64(off)
                if off + B > 64:
                    words[:, w + 1] |= fields[:, j] >> np.uint64(64 - off)
            offset = half * (((1 << (S * B)) - 1) // ((1 << B) - 1))
            raw, width = words.tobytes(), 8 * n_words
            ms = [(int.from_bytes(raw[b * width:(b + 1) * width], "little") - offset) % n for b in range(rows)]
        else:
            xs = mantissas.tolist() if isinstance(mantissas, np.ndarray) else mantissas
            ms = [sum(x << (B * j) for j, x in enumerate(xs[b * S:(b + 1) * S])) % n for b in range(rows)]
        return _native.ints_to_limbs(ms, n_limbs)

    def segment_ids(self, ids, num_segments=None):
        """Segment ids for EncryptedVector.segment_sum under this key, validated once and kept on the device ->
        ResidentSegmentIds.  ids: integers of shape (rows,) or (F, rows) in [-1, num_segments) (num_segments defaults to
        max + 1; TypeError / ValueError as segment_sum raises them).  The bins of a training set stay the same from node to
        node: pass the object in place of the ids and, from the sizes on at which the plan is made on the device, only the
        `node` array of a call crosses PCIe.  The upload happens on first use, once per device of a fleet."""
        from .ciphertext import ResidentSegmentIds
        return ResidentSegmentIds(self, ids, num_segments)

    def encrypt_packed(self, values, slots, slot_bits, precision=None, r_values=None, device=False, rho_values=None):
        """Encode, PACK and encrypt -> EncryptedVector of ceil(len(values) / slots) rows: row b encrypts
        V_b = x[b*S] + x[b*S + 1] * 2^B + x[b*S + 2] * 2^(2B) + ... (S = slots, B = slot_bits) for the signed mantissas x of the
        values — what EncryptedVector.pack(S, B) makes of encrypt_batch(values), for one encryption per S values instead of S
        encryptions and a packing step (BatchCrypt-style batching of quantised gradients; the "g, h packing" of federated
        boosting).  Such rows add slot by slot (`+`), scale every slot (`* k`), go through segment_sum / cumsum / pack, and are
        read back by PaillierPrivateKey.decrypt_packed(vector, S, B, count=len(values)).
        Every value is encoded as EncodedNumber.encode(self, v, precision=precision) encodes it (signed mantissa and exponent)
        and all exponents must agree (ValueError naming the first index that differs): integers give exponent 0, floats need a
        `precision`.  int64 / float64 arrays and homogeneous lists are encoded by numpy with the same mantissas element for
        element (an exact power-of-two scaling, then rounding half to even).  A mantissa outside [-2^(B-1), 2^(B-1)) raises
        ValueError with its index.  slots / slot_bits are checked as EncryptedVector.pack checks them: not an integer —
        TypeError, below 1 — ValueError, slots * slot_bits > max_int.bit_length() - 1 — ValueError.
        Row b is bit for bit raw_encrypt(V_b mod n, r_b); r_values, rho_values (one per packed ROW), the obfuscator pool and
        device=True behave as in encrypt_batch.  The plaintext rows are formed on the GPU (Engine.slots_pack_dev: shifts and one reduction mod n, a
        memory-bound kernel) and stay there; without that kernel, or for slot_bits > 64, they are formed on the host: same bits.
        WHAT CANNOT BE CHECKED UNDER ENCRYPTION (EncryptedVector.pack): a slot whose true value, after every later addition or
        scaling of packed vectors, leaves [-2^(B-1), 2^(B-1)) spills into its neighbour, silently.  Choosing slot_bits with
        enough headroom for the sums to come is the caller's job."""
        from .ciphertext import EncryptedVector
        from ._device import DeviceArray
        for name, value in (("slots", slots), ("slot_bits", slot_bits)):
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
                raise TypeError("%s must be an integer" % name)
            if value < 1:
                raise ValueError("%s must be at least 1" % name)
        S, B = int(slots), int(slot_bits)
        bound = self.max_int.bit_length() - 1
        if S * B > bound:
            raise ValueError("slots * slot_bits = %d bits do not fit the %d bits a plaintext of this key holds" % (S * B, bound))
        mant, exponent = self._packed_mantissas(values, precision)
        count = len(mant)
        lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
        if count and isinstance(mant, np.ndarray):
            if B < 64 and (int(mant.min()) < lo or int(mant.max()) > hi):
                i = int(np.flatnonzero((mant < lo) | (mant > hi))[0])
                raise ValueError("the mantissa %d at index %d does not fit a slot of %d bits" % (mant[i], i, B))
        else:
            for i, x in enumerate(mant):
                if not lo <= x <= hi:
                    raise ValueError("the mantissa %d at index %d does not fit a slot of %d bits" % (x, i, B))
        eng = self._get_engine()
        rows = -(-count // S)
        exps = np.full(rows, exponent, dtype=np.int64)
        fresh = r_values is None and rho_values is None
        rho = self._rho_limbs(rho_values, rows, r_values) if rho_values is not None else None
        if rows == 0:
            empty = DeviceArray(eng.ctx, 0, eng.ct_limbs) if device else np.zeros((0, eng.ct_limbs), dtype=np.uint32)
            return EncryptedVector(self, empty, exps, obfuscated=fresh)
        resident = isinstance(mant, np.ndarray) and B <= 64 and eng.has_slot_codec()
        m = eng.slots_pack_dev(mant, S, B) if resident else self._pack_plain_host(mant, S, B)
        limbs = None
        if rho is not None or (fresh and self._short is not None and not hasattr(eng.ctx, "encrypt_dev")):
            if rho is None:
                rho = self._draw_rho(eng, rows)
            if device or resident:
                limbs = eng.short_pow_dev(rho, m=m)
                if not device:
                    limbs = limbs.to_host()
            else:
                limbs = eng.short_pow(rho, m=m)
        elif fresh and hasattr(eng.ctx, "encrypt_dev"):
            limbs = eng.encrypt_from_obfuscators(m)                 # the pool made by precompute_obfuscators (each used once)
            if limbs is None and rows <= SCALAR_POOL_REFILL // 4:
                eng.fill_obfuscator_pool(SCALAR_POOL_REFILL)
                limbs = eng.encrypt_from_obfuscators(m)
            if limbs is None:
                limbs = eng.raw_encrypt_fresh(m, device)
            elif not device:
                limbs = limbs.to_host()
        else:
            if fresh:
                r = random_lt_n_limbs(self.n, rows, eng.n_limbs)
            else:
                r = r_values if isinstance(r_values, np.ndarray) else list(r_values)
                if len(r) != rows:
                    raise ValueError("%d r_values for %d packed rows" % (len(r), rows))
            if device or resident:
                limbs = eng.raw_encrypt_dev(m, r)
                if not device:
                    limbs = limbs.to_host()
            else:
                limbs = eng.raw_encrypt(m, r)
        return EncryptedVector(self, limbs, exps, obfuscated=fresh)

    def encrypt_batch_sharded(self, values, precision=None):
        """encrypt_batch with the ciphertexts left RESIDENT, one EncryptedVector per device of the fleet (contiguous shards in
        order; a single vector on the ordinary device when no fleet is configured): the per-device list form of the fan-out.
        Each vector is operated on by the engine of its own device; `PaillierPrivateKey.decrypt_batch` takes the list."""
        from .ciphertext import EncryptedVector
        eng = self._get_engine()
        fl = self._get_fleet()
        if fl is None or not hasattr(eng.ctx, "encrypt_dev"):
            return [self.encrypt_batch(values, precision, device=hasattr(eng.ctx, "encrypt_dev"))]
        signed = EncodedNumber.encode_signed(values, precision) if eng.n_limbs >= 4 else None
        if signed is not None:
            mag, neg, exps = signed
            m = EncodedNumber.signed_to_limbs(self, mag, neg, eng.n_limbs)
        else:
            m, exps = EncodedNumber.encode_many(self, values, precision)
            m = m if isinstance(m, np.ndarray) else eng.plain_limbs([v % self.n for v in m])
        exps = np.asarray(exps, dtype=np.int64)

        def shard(e, lo, hi):
            self._short_sync(e)
            got = e.encrypt_from_obfuscators(m[lo:hi])
            return got if got is not None else e.raw_encrypt_fresh(m[lo:hi], True)
        bounds = fl.shards(len(exps), min_rows=1)
        parts = fl.run(len(exps), shard, min_rows=1)
        return [EncryptedVector(self, part, exps[lo:hi], obfuscated=True) for part, (lo, hi) in zip(parts, bounds)]


class PaillierPrivateKey(object):
    def __init__(self, public_key, p, q):
        if not p * q == public_key.n:
            raise ValueError('given public key does not match the given p and q.')
        if p == q:
            raise ValueError('p and q have to be different')
        self.public_key = public_key
        self.p, self.q = (q, p) if q < p else (p, q)
        self.psquare = self.p * self.p
        self.qsquare = self.q * self.q
        self.p_inverse = util.invert(self.p, self.q)
        if public_key.g == public_key.n + 1:
            # h_function in closed form: g = 1 + n and n^2 = 0 (mod p^2), so g^(p-1) = 1 + (p-1) n = 1 + p (-q mod p)
            # (mod p^2), L(.) = -q mod p and hp = (-q)^-1 mod p — the value phe/paillier.py:356-360 computes with a
            # modular exponentiation (pinned to the reference's numbers by tests/test_api.py and the golden fixtures)
            self.hp = util.invert((-self.q) % self.p, self.p)
            self.hq = util.invert((-self.p) % self.q, self.q)
        else:
            self.hp = self.h_function(self.p, self.psquare)
            self.hq = self.h_function(self.q, self.qsquare)
        self._engine = None
        self._engine_lock = threading.Lock()

    @staticmethod
    def from_totient(public_key, totient):
        p_plus_q = public_key.n - totient + 1
        p_minus_q = util.isqrt(p_plus_q * p_plus_q - public_key.n * 4)
        q = (p_plus_q - p_minus_q) // 2
        p = p_plus_q - q
        if not p * q == public_key.n:
            raise ValueError('given public key and totient do not match.')
        return PaillierPrivateKey(public_key, p, q)

    def _get_engine(self):
        eng = self._engine
        if eng is not None:
            return eng
        with self._engine_lock:
            if self._engine is None:
                fresh = Engine(self.public_key.n, self.p, self.q, self.hp, self.hq, self.p_inverse)
                # The public key of a key pair works through the private key's engine from here on: one GPU context per key
                # pair, and encryptions under it take the key owner's CRT form (Engine.owner_encrypt: same ciphertext bits,
                # about half the work).  Obfuscators made ahead of time stay where they are: the new engine adopts the old
                # engine's pool OBJECT (device pointers are valid across contexts), so a thread that is still inside the old
                # engine and a thread inside the new one take rows under the same lock — nothing is handed out twice.
                pub = self.public_key
                with pub._engine_lock:
                    old = pub._engine
                    if old is not None and old is not fresh:
                        fresh._obf = old._obf
                    pub._engine = fresh
                    # the further devices of a fleet get key-pair engines too (built on first use), each with a pool of its own
                    n, p, q, hp, hq, pinv = pub.n, self.p, self.q, self.hp, self.hq, self.p_inverse
                    pub._fleet_factory = lambda device: Engine(n, p, q, hp, hq, pinv, device=device)
                    old_fleet, pub._fleet = pub._fleet, None
                    if old_fleet is not None:
                        # the public key already fanned out (encrypt_batch_sharded / precompute_obfuscators before the first
                        # private-key call): its resident parts live on devices 1..k and its pools hold obfuscators there.
                        # The key pair's fleet is built NOW, engine for engine on the same devices, each adopting the pool of
                        # the engine it replaces; the old contexts resolve to their successors (Fleet.succeed)
                        from . import fleet
                        pub._fleet = fleet.Fleet(fresh, pub._fleet_factory, old_fleet.devices).succeed(old_fleet)
                self._engine = fresh
            return self._engine

    def _get_fleet(self):
        """the key pair's fleet (PaillierPublicKey._get_fleet): every engine of it holds the private key"""
        self._get_engine()
        return self.public_key._get_fleet()

    def __repr__(self):
        return "<PaillierPrivateKey for {}>".format(repr(self.public_key))

    def __eq__(self, other):
        return self.p == other.p and self.q == other.q

    def __hash__(self):
        return hash((self.p, self.q))

    def __getstate__(self):
        return {"n": self.public_key.n, "p": self.p, "q": self.q}

    def __setstate__(self, state):
        self.__init__(PaillierPublicKey(state["n"]), state["p"], state["q"])

    # once-per-key helpers, host integers (phe/paillier.py:356-364)
    def h_function(self, x, xsquare):
        return util.invert(self.l_function(util.powmod(self.public_key.g, x - 1, xsquare), x), x)

    def l_function(self, x, p):
        return (x - 1) // p

    def crt(self, mp, mq):
        u = (mq - mp) * self.p_inverse % self.q
        return mp + u * self.p

    # ---- scalar API ---------------------------------------------------------------------------------
    def raw_decrypt(self, ciphertext):
        if not isinstance(ciphertext, int):
            raise TypeError('Expected ciphertext to be an int, not: %s' % type(ciphertext))
        return self.raw_decrypt_batch([ciphertext])[0]

    def decrypt(self, encrypted_number):
        return self.decrypt_encoded(encrypted_number).decode()

    def decrypt_encoded(self, encrypted_number, Encoding=None):
        from .ciphertext import EncryptedNumber
        if not isinstance(encrypted_number, EncryptedNumber):
            raise TypeError('Expected encrypted_number to be an EncryptedNumber not: %s' % type(encrypted_number))
        if self.public_key != encrypted_number.public_key:
            raise ValueError('encrypted_number was encrypted against a different key!')
        if Encoding is None:
            Encoding = EncodedNumber
        encoded = self.raw_decrypt(encrypted_number.ciphertext(be_secure=False))
        return Encoding(self.public_key, encoded, encrypted_number.exponent)

    # ---- batched API ----------------------------------------------------------------------------------
    def raw_decrypt_batch(self, ciphertexts):
        ciphertexts = list(ciphertexts)
        for c in ciphertexts:
            if not isinstance(c, int):
                raise TypeError('Expected ciphertext to be an int, not: %s' % type(c))
        eng = self._get_engine()
        # ciphertexts are residues mod n^2; reduce stray larger ints exactly like powmod would
        return eng.to_ints(eng.raw_decrypt([c % self.public_key.nsquare for c in ciphertexts]))

    def decrypt_batch(self, vector, Encoding=None, as_array=False):
        """EncryptedVector (or list of EncryptedNumber) -> list of decoded ints/floats.
        as_array=True returns a numpy array instead — np.int64 when every exponent is 0, np.float64 when every exponent is
        negative — and raises ValueError where that form does not apply: a custom Encoding, exponents of both kinds or positive
        ones.  The values are those of the list; a row in the overflow gap raises OverflowError('Overflow detected in decrypted
        number'), an integer outside int64 OverflowError, a plaintext >= n the corrupted-number ValueError, and the lowest row
        index decides which.  With the value codec kernels (Engine.has_value_codec) and exponents of -240 or more the decode
        kernel runs behind each chunk's decrypt (Engine.raw_decrypt_decode_chunks): 8 bytes and a status byte per row come
        down instead of limb rows."""
        if as_array:
            return self._decrypt_batch_array(vector, Encoding)
        from .ciphertext import EncryptedVector
        if isinstance(vector, (list, tuple)) and vector and all(isinstance(v, EncryptedVector) for v in vector):
            # the per-device list of encrypt_batch_sharded: every part on the engine of its own device, concurrently
            fl = self._get_fleet()
            if fl is None or len(vector) == 1:
                return [x for v in vector for x in self.decrypt_batch(v, Encoding)]
            import concurrent.futures as cf
            with cf.ThreadPoolExecutor(len(vector)) as pool:
                return [x for part in pool.map(lambda v: self.decrypt_batch(v, Encoding), vector) for x in part]
        if not isinstance(vector, EncryptedVector):
            vector = EncryptedVector.from_numbers(self.public_key, vector)
        if self.public_key != vector.public_key:
            raise ValueError('encrypted_number was encrypted against a different key!')
        eng = self._get_engine()
        plain_decode = Encoding is None or Encoding is EncodedNumber
        fl = self._get_fleet()
        if vector.on_device and fl is not None:
            eng = self.public_key._engine_for(vector._store)       # a resident vector is decrypted where it lives
        if not vector.on_device and fl is not None and len(fl.shards(len(vector))) > 1:
            # single-process fan-out: contiguous shards of the host vector, one device each, decoded in shard order
            limbs, exps = vector.limbs(be_secure=False), vector.exponent_array

            def shard(e, lo, hi):
                plain = e.raw_decrypt(limbs[lo:hi])
                if plain_decode:
                    return EncodedNumber.decode_limbs(self.public_key, plain, exps[lo:hi])
                return Encoding.decode_many(self.public_key, e.to_ints(plain), exps[lo:hi].tolist())
            return [x for part in fl.run(len(vector), shard) for x in part]
        if vector.on_device or hasattr(eng.ctx, "decrypt_dev"):
            # chunks: the download and decoding of one chunk (and, for a host vector, the upload of the next) overlap
            # the kernels; device pointers are valid across contexts of the same GPU
            out, exps = [], vector.exponent_array
            limbs = vector.limbs(be_secure=False)
            chunks = eng.raw_decrypt_dev_chunks(limbs) if vector.on_device else eng.raw_decrypt_host_chunks(limbs)
            for lo, hi, plain in chunks:
                if plain_decode:
                    out += EncodedNumber.decode_limbs(self.public_key, plain, exps[lo:hi])
                else:
                    out += Encoding.decode_many(self.public_key, eng.to_ints(plain), exps[lo:hi].tolist())
            return out
        plain = eng.raw_decrypt(vector.limbs(be_secure=False))
        if plain_decode:
            return EncodedNumber.decode_limbs(self.public_key, plain, vector.exponent_array)
        return Encoding.decode_many(self.public_key, eng.to_ints(plain), vector.exponents)

    def _decrypt_batch_array(self, vector, Encoding):
        """decrypt_batch(as_array=True)"""
        from .ciphertext import EncryptedVector
        if isinstance(vector, (list, tuple)) and vector and all(isinstance(v, EncryptedVector) for v in vector):
            # the per-device list of encrypt_batch_sharded, part after part: the lowest row decides which exception is raised
            parts = [self._decrypt_batch_array(v, Encoding) for v in vector]
            kinds = {part.dtype for part, v in zip(parts, vector) if len(v)}
            if len(kinds) > 1:
                raise ValueError("as_array needs exponents that are all 0 (int64) or all negative (float64)")
            dtype = kinds.pop() if kinds else np.dtype(np.int64)
            return np.concatenate([part.astype(dtype, copy=False) for part in parts])
        if not isinstance(vector, EncryptedVector):
            vector = EncryptedVector.from_numbers(self.public_key, vector)
        if self.public_key != vector.public_key:
            raise ValueError('encrypted_number was encrypted against a different key!')
        if not (Encoding is None or Encoding is EncodedNumber):
            raise ValueError("as_array does not apply to a custom Encoding")
        pk = self.public_key
        exps = vector.exponent_array
        all_int, all_float = bool((exps == 0).all()), bool(len(exps) and (exps < 0).all())
        if not (all_int or all_float):
            raise ValueError("as_array needs exponents that are all 0 (int64) or all negative (float64)")
        dtype = np.int64 if all_int else np.float64
        if len(vector) == 0:
            return np.zeros(0, dtype=dtype)
        eng = self._get_engine()
        fl = self._get_fleet()
        if vector.on_device and fl is not None:
            eng = self.public_key._engine_for(vector._store)
        fanned_out = not vector.on_device and fl is not None and len(fl.shards(len(vector))) > 1
        parts = []
        if EncodedNumber.BASE == 16 and int(exps.min()) >= -240 and not fanned_out and eng.has_value_codec():
            kind = 0 if all_int else 1
            chunks = eng.raw_decrypt_decode_chunks(vector.limbs(be_secure=False), kind, exps if kind else None)
            for lo, hi, words, status, fetch in chunks:
                bad = np.flatnonzero(status)
                if len(bad):
                    # in row order: the rows the host must decode (status 2 of the float kind) up to the first row that raises
                    stop = next((int(i) for i in bad if not (kind == 1 and status[i] == 2)), None)
                    redo = [int(i) for i in bad if stop is None or i < stop]
                    if redo:
                        plain = eng.to_ints(fetch(redo))
                        vals = words.view(np.float64)
                        for i, m in zip(redo, plain):
                            vals[i] = EncodedNumber(pk, m, int(exps[lo + i])).decode()
                    if stop is not None:
                        if status[stop] == 1:
                            raise OverflowError('Overflow detected in decrypted number')
                        if status[stop] == 3:
                            raise ValueError('Attempted to decode corrupted number')
                        raise OverflowError('the integer at index %d does not fit int64' % (lo + stop))
                parts.append(words.view(dtype))
            return parts[0] if len(parts) == 1 else np.concatenate(parts)
        # the list route, chunk by chunk, into the same array
        for lo, hi, plain in self._raw_plain_chunks(vector):
            try:
                vals = EncodedNumber.decode_limbs(pk, plain, exps[lo:hi])
                failed = False
            except (OverflowError, ValueError):
                failed = True
            if failed:                                                 # row by row: the lowest row decides what is raised
                vals = []
                for m, e in zip(eng.to_ints(plain), exps[lo:hi].tolist()):
                    vals.append(EncodedNumber(pk, m, e).decode())
                    if all_int and not -(1 << 63) <= vals[-1] < 1 << 63:
                        raise OverflowError('the integer at index %d does not fit int64' % (lo + len(vals) - 1))
            try:
                parts.append(np.asarray(vals, dtype=dtype))
            except OverflowError:
                i = next(i for i, v in enumerate(vals) if not -(1 << 63) <= v < 1 << 63)
                raise OverflowError('the integer at index %d does not fit int64' % (lo + i)) from None
        return parts[0] if len(parts) == 1 else np.concatenate(parts)

    def _raw_plain_chunks(self, vector):
        """(lo, hi, plaintext limb rows on the host) over an EncryptedVector, by the raw decrypt paths of decrypt_batch:
        resident or host, in chunks whose download overlaps the kernels of the next"""
        eng = self._get_engine()
        fl = self._get_fleet()
        if vector.on_device and fl is not None:
            eng = self.public_key._engine_for(vector._store)
        limbs = vector.limbs(be_secure=False)
        if not vector.on_device and fl is not None and len(fl.shards(len(vector))) > 1:
            lo = 0
            for plain in fl.run(len(vector), lambda e, lo, hi: e.raw_decrypt(limbs[lo:hi])):   # (contiguous shards, in order)
                yield lo, lo + len(plain), plain
                lo += len(plain)
        elif vector.on_device or hasattr(eng.ctx, "decrypt_dev"):
            chunks = eng.raw_decrypt_dev_chunks(limbs) if vector.on_device else eng.raw_decrypt_host_chunks(limbs)
            for lo, hi, plain in chunks:
                yield lo, hi, plain
        elif len(vector):
            yield 0, len(vector), eng.raw_decrypt(limbs)

    def decrypt_packed(self, vector, slots, slot_bits, count=None, Encoding=None, as_array=False):
        """The values of a vector packed by EncryptedVector.pack(slots, slot_bits) (and of sums of such vectors) -> list of
        decoded ints / floats, like decrypt_batch: ONE decrypt per `slots` values.  Value number b * slots + j is slot j of
        row b.  The rows are decrypted through the raw decrypt paths of decrypt_batch; each plaintext m is unpacked on the host:
        v = m if m <= max_int, m - n if m >= n - max_int (in between: OverflowError, as EncodedNumber.decode); slot by slot
        d_j = ((v + 2^(B-1)) mod 2^B) - 2^(B-1), v <- (v - d_j) >> B; what is left of v after the last slot must be 0
        (OverflowError: the packed value did not fit slots * slot_bits bits).  d_j is decoded as
        Encoding(public_key, d_j % n, exponent of row b).decode().  count keeps the first `count` values (default
        len(vector) * slots; outside [0, len(vector) * slots]: ValueError).
        as_array=True returns a numpy array instead of the list — np.int64 when every exponent is 0, np.float64 when every
        exponent is negative, cut to `count` — and raises ValueError where that form does not apply: slot_bits > 64, a custom
        Encoding, or exponents of both kinds.
        With the slot codec kernels (Engine.has_slot_codec), slot_bits <= 64, the default Encoding and exponents of one kind,
        the unpack kernel runs behind each chunk's decrypt (Engine.raw_decrypt_unpack_chunks): int64 values and one status byte
        per row come down instead of limb rows.  Same values, same exceptions, and the lowest row index decides which is raised.
        A slot that left [-2^(B-1), 2^(B-1)) before it was decrypted has spilled into its neighbour and cannot be told from a
        legitimate value: see EncryptedVector.pack."""
        from .ciphertext import EncryptedVector
        for name, value in (("slots", slots), ("slot_bits", slot_bits)):
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
                raise TypeError("%s must be an integer" % name)
            if value < 1:
                raise ValueError("%s must be at least 1" % name)
        slots, slot_bits = int(slots), int(slot_bits)
        if not isinstance(vector, EncryptedVector):
            vector = EncryptedVector.from_numbers(self.public_key, vector)
        if self.public_key != vector.public_key:
            raise ValueError('encrypted_number was encrypted against a different key!')
        total = len(vector) * slots
        if count is None:
            count = total
        if isinstance(count, (bool, np.bool_)) or not isinstance(count, (int, np.integer)):
            raise TypeError("count must be an integer")
        count = int(count)
        if not 0 <= count <= total:
            raise ValueError("count must lie in [0, %d]" % total)
        plain_decode = Encoding is None or Encoding is EncodedNumber
        exps = vector.exponent_array
        all_int, all_float = bool((exps == 0).all()), bool(len(exps) and (exps < 0).all())
        if as_array:
            if slot_bits > 64:
                raise ValueError("as_array needs slot_bits <= 64: a wider slot does not fit int64")
            if not plain_decode:
                raise ValueError("as_array does not apply to a custom Encoding")
            if not (all_int or all_float):
                raise ValueError("as_array needs exponents that are all 0 (int64) or all negative (float64)")
        log2b = int(round(EncodedNumber.LOG2_BASE))
        eng = self._get_engine()
        fl = self._get_fleet()
        if vector.on_device and fl is not None:
            eng = self.public_key._engine_for(vector._store)
        fanned_out = not vector.on_device and fl is not None and len(fl.shards(len(vector))) > 1
        if (len(vector) and plain_decode and slot_bits <= 64 and (all_int or all_float) and (1 << log2b) == EncodedNumber.BASE
                and int(exps.min()) * log2b >= -960 and not fanned_out and eng.has_slot_codec()
                and (as_array or PACKED_LISTS_THROUGH_CODEC)):
            parts = []
            for lo, hi, values, status in eng.raw_decrypt_unpack_chunks(vector.limbs(be_secure=False), slots, slot_bits):
                bad = np.flatnonzero(status)
                if len(bad):
                    if status[bad[0]] == 1:
                        raise OverflowError('Overflow detected in decrypted number')
                    raise OverflowError('a packed value does not fit %d slots of %d bits' % (slots, slot_bits))
                parts.append(values)
            vals = (parts[0] if len(parts) == 1 else np.concatenate(parts))[:count]
            if all_float:
                # correctly rounded int64 -> float64, then an exact power-of-two scaling = the reference's true division
                vals = np.ldexp(vals.astype(np.float64), np.repeat(exps, slots)[:count] * log2b)
            return vals if as_array else vals.tolist()
        out = []
        for lo, hi, plain in self._raw_plain_chunks(vector):
            out.append(self._unpack_plain(plain, exps[lo:hi], slots, slot_bits, None if plain_decode else Encoding, as_array))
        if as_array:
            out = [np.asarray(part, dtype=np.int64 if all_int else np.float64) for part in out]
            return np.concatenate(out)[:count] if out else np.zeros(0, dtype=np.int64 if all_int else np.float64)
        out = [x for part in out for x in part]
        del out[count:]
        return out

    def _unpack_plain(self, plain, exps, slots, slot_bits, Encoding, as_array=False):
        """the decoded slots of the plaintext rows `plain` (host limbs), row after row (decrypt_packed).  With
        u = v + sum_j 2^(B-1) 2^(B j) the slots are the B-bit digits of u less 2^(B-1), and v fits slots * B bits exactly when
        0 <= u < 2^(slots * B): one Python integer per ROW; for B <= 64 the digits are cut out of the rows' 64-bit words by
        numpy, `slots` vector operations whatever the number of rows (as_array: those values as the numpy array they are)."""
        from . import _native
        pk = self.public_key
        n, max_int = pk.n, pk.max_int
        S, B = slots, slot_bits
        half = 1 << (B - 1)
        offset = half * (((1 << (S * B)) - 1) // ((1 << B) - 1))     # 2^(B-1) in every slot
        us = []
        for m in _native.limbs_to_ints(plain):
            if m <= max_int:
                v = m
            elif m >= n - max_int:
                v = m - n
            else:
                raise OverflowError('Overflow detected in decrypted number')
            u = v + offset
            if u < 0 or u >> (S * B):
                raise OverflowError('a packed value does not fit %d slots of %d bits' % (S, B))
            us.append(u)
        rows = len(us)
        row_exps = np.repeat(np.asarray(exps, dtype=np.int64), S)
        if rows == 0:
            return []
        log2b = int(round(EncodedNumber.LOG2_BASE))
        one_kind = bool((row_exps == 0).all() or (row_exps < 0).all())
        if (Encoding is None and B <= 64 and (1 << log2b) == EncodedNumber.BASE and one_kind
                and int(row_exps.min()) * log2b >= -960):
            n_words = (S * B + 63) // 64 + 1                         # (one spare word: a digit may straddle the last one)
            words = np.frombuffer(b"".join(u.to_bytes(8 * n_words, "little") for u in us), dtype=np.uint64).reshape(rows, n_words)
            digits = np.empty((rows, S), dtype=np.uint64)
            mask = np.uint64((1 << B) - 1)
            for j in range(S):
                w, off = divmod(B * j, 64)
                d = words[:, w] >> np.uint64(off)
                if off + B > 64:
                    d = d | (words[:, w + 1] << np.uint64(64 - off))
                digits[:, j] = d & mask
            if B == 64:
                vals = (digits ^ np.uint64(half)).view(np.int64)     # digit - 2^63 in two's complement
            else:
                vals = digits.view(np.int64) - np.int64(half)
            vals = vals.reshape(-1)
            if row_exps[0] < 0:
                # correctly rounded int64 -> float64, then an exact power-of-two scaling = the reference's true division
                vals = np.ldexp(vals.astype(np.float64), row_exps * log2b)
            return vals if as_array else vals.tolist()
        mask = (1 << B) - 1
        cls = EncodedNumber if Encoding is None else Encoding
        out = []
        for u, e in zip(us, np.asarray(exps, dtype=np.int64).tolist()):
            for j in range(S):
                out.append(cls(pk, (((u >> (B * j)) & mask) - half) % n, e).decode())
        return out


class PaillierPrivateKeyring(Mapping):
    def __init__(self, private_keys=None):
        private_keys = private_keys or []
        self.__keyring = {k.public_key: k for k in private_keys}

    def __getitem__(self, key):
        return self.__keyring[key]

    def __len__(self):
        return len(self.__keyring)

    def __iter__(self):
        return iter(self.__keyring)

    def __delitem__(self, public_key):
        del self.__keyring[public_key]

    def add(self, private_key):
        if not isinstance(private_key, PaillierPrivateKey):
            raise TypeError("private_key should be of type PaillierPrivateKey, not %s" % type(private_key))
        self.__keyring[private_key.public_key] = private_key

    def decrypt(self, encrypted_number):
        return self.__keyring[encrypted_number.public_key].decrypt(encrypted_number)
