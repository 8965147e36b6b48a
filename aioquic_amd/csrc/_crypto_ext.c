/*
 * aioquic_amd._crypto -- CPython binding of libquicpp.so (include/quic_pp.h).
 *
 * Built like the reference's aioquic._crypto: limited API 3.10 (abi3) and
 * heap types from PyType_FromSpec (src/aioquic/_crypto.c:203-219,358-372,
 * setup.py:30-39), so one binary serves every CPython >= 3.10.
 *
 * Object API identical to the reference (src/aioquic/_crypto.pyi:1-15):
 *   AEAD(cipher_name, key, iv).encrypt(data, associated_data, packet_number) -> bytes
 *                             .decrypt(data, associated_data, packet_number) -> bytes
 *   HeaderProtection(cipher_name, key).apply(plain_header, protected_payload) -> bytes
 *                                     .remove(packet, encrypted_offset) -> (bytes, int)
 *   CryptoError(ValueError), with the reference's messages (_crypto.c:17-29,79-90,126-152).
 * Every byte of crypto runs on the GPU through libquicpp; there is no CPU path.
 * Without a gfx950 device the constructors raise RuntimeError.
 *
 * Batch API (pointers are ints: device pointers for the device forms, host
 * pointers for the *_into forms; the caller keeps the memory alive):
 *   KeyTable(capacity) .set(materials) .derive(secrets) .derive_initial(records)
 *                      .derive_next(records) .derive_trace(enable) .clear(slots) .capacity
 *   aead_deferred(cipher_name, key, iv)             an AEAD whose device table waits for its first use
 *   Plan(capacity)                                  device scratch of the bucketing step
 *   protect(table, desc_ptr, n, in_ptr, out_ptr, res_ptr, stream[, plan])   -> None
 *   unprotect(...)                                                          -> None
 *   plan_build(plan, table, desc_ptr, n, stream)    bucket a batch by (suite, slot)
 *   protect_host(table, desc, data, out_len) -> (bytes out, bytes results)
 *   unprotect_host(table, desc, data, out_len) -> (bytes out, bytes results)
 *   protect_into(table, desc_ptr, n, in_ptr, in_len, out_ptr, out_len, res_ptr) -> None
 *   unprotect_into(...)                                                         -> None
 *   hp_mask_host(table, slots, samples) -> bytes
 *   protect_datagrams(...), unprotect_walk(...)     the batched callers' C paths
 *   MultiSession(devices, key_capacity)             one host batch over several GPUs
 *   CidMap(capacity) .put(records) .remove(records) .find(cid) .home(cid) .count .buckets
 *   route(map, cid_len, off_ptr, len_ptr, n, in_ptr, slot_ptr, exp_ptr, n_conn, flags,
 *         desc_ptr, route_ptr, stream)              raw datagrams -> descriptors, by connection ID
 *   route_unprotect_host(table, map, cid_len, offs, lens, data, conn_slot, conn_expected,
 *                        flags, out_len) -> (out, desc, route, results)
 *   receive_routed(...)                             receive.receive_routed's C path
 *   route_reply(...), receive_accept_reply(...)     Retry / Version Negotiation replies built on the device
 *   route_token(...), route_accept_tokens(...), receive_serve(...)   Retry tokens validated on the device
 *   route_accept(...), receive_accept(...)          unrouted Initials accepted on the device:
 *                                                   the device form, receive.accept_routed's C path
 *
 * Threads: host-buffer calls release the GIL.  Each OS thread gets its own
 * qpp_session (pinned staging + streams; quic_pp.h: a session is single-
 * threaded), created on first use and destroyed when the thread exits, so
 * concurrent calls from different threads never share staging.
 */
#define PY_SSIZE_T_CLEAN
#define Py_LIMITED_API 0x030A0000
#include <Python.h>
#include <ctype.h>
#include <pthread.h>
#include <stdarg.h>
#include <string.h>

#include "quic_pp.h"
#include "qpp_rxwalk.h"

static PyObject *g_crypto_error;
static PyObject *g_aead_type, *g_hp_type, *g_kt_type, *g_plan_type, *g_multi_type, *g_cidmap_type;
/* what the receive walks' records are made of: b"", -1, 0 and the drop reasons (module init) */
static PyObject *g_empty, *g_minus1, *g_zero, *g_s_key, *g_s_dec, *g_s_rsv, *g_s_closed;

/* ------------------------------------------------------------ sessions -- */

static pthread_key_t g_session_key;
static pthread_once_t g_session_once = PTHREAD_ONCE_INIT;

static void session_free(void *s) { qpp_session_destroy((qpp_session *)s); }
static void session_key_init(void) { (void)pthread_key_create(&g_session_key, session_free); }

/* This thread's session, created on first use.  Call with the GIL held. */
static qpp_session *session(void)
{
    (void)pthread_once(&g_session_once, session_key_init);
    qpp_session *s = (qpp_session *)pthread_getspecific(g_session_key);
    if (s) return s;
    int rc = qpp_session_create(1 << 16, 64, &s);
    if (rc != QPP_OK) {
        PyErr_Format(PyExc_RuntimeError, "aioquic_amd: cannot open a gfx950 session (%s)",
                     qpp_strerror(rc));
        return NULL;
    }
    if (pthread_setspecific(g_session_key, s) != 0) {
        qpp_session_destroy(s);
        PyErr_SetString(PyExc_RuntimeError, "aioquic_amd: cannot store the thread's session");
        return NULL;
    }
    return s;
}

static int check_rc(int rc)
{
    if (rc == QPP_OK) return 0;
    PyErr_Format(PyExc_RuntimeError, "aioquic_amd: %s", qpp_strerror(rc));
    return -1;
}

static void *as_ptr(unsigned long long v) { return (void *)(uintptr_t)v; }

static void heap_dealloc(PyObject *self)
{
    PyTypeObject *tp = Py_TYPE(self);
    freefunc f = (freefunc)PyType_GetSlot(tp, Py_tp_free);
    f(self);
    Py_DECREF(tp);
}

/* --------------------------------------------------------- cipher names -- */

static int streq_ci(const char *a, Py_ssize_t alen, const char *b)
{
    if ((size_t)alen != strlen(b)) return 0;
    for (Py_ssize_t i = 0; i < alen; ++i)
        if (tolower((unsigned char)a[i]) != b[i]) return 0;
    return 1;
}

/* EVP cipher names the reference maps to each suite (quic/crypto.py:12-16) */
static int aead_suite(const char *name, Py_ssize_t len)
{
    if (streq_ci(name, len, "aes-128-gcm") || streq_ci(name, len, "id-aes128-gcm")) return QPP_AES_128_GCM;
    if (streq_ci(name, len, "aes-256-gcm") || streq_ci(name, len, "id-aes256-gcm")) return QPP_AES_256_GCM;
    if (streq_ci(name, len, "chacha20-poly1305")) return QPP_CHACHA20_POLY1305;
    return -1;
}

static int hp_suite(const char *name, Py_ssize_t len)
{
    if (streq_ci(name, len, "aes-128-ecb")) return QPP_AES_128_GCM;
    if (streq_ci(name, len, "aes-256-ecb")) return QPP_AES_256_GCM;
    if (streq_ci(name, len, "chacha20")) return QPP_CHACHA20_POLY1305;
    return -1;
}

static int suite_key_len(int suite) { return suite == QPP_AES_128_GCM ? 16 : 32; }

/* --------------------------------------------------- parallel host copy -- */

/* Many (dst, src, len) copies between caller memory and pinned staging, split
 * over up to 8 threads by bytes (one thread streams ~6-10 GB/s, well under
 * the PCIe rate).  Small totals stay on the calling thread.  Call without the
 * GIL only when every buffer is kept alive by the caller. */
typedef struct {
    uint8_t **dst;
    const uint8_t **src;
    const size_t *len;
    size_t b, e;
} CopyJob;

static void *copy_job(void *arg)
{
    CopyJob *j = (CopyJob *)arg;
    for (size_t i = j->b; i < j->e; ++i) memcpy(j->dst[i], j->src[i], j->len[i]);
    return NULL;
}

static void par_copy(uint8_t **dst, const uint8_t **src, const size_t *len, size_t n, size_t total)
{
    enum { kThreads = 8 };
    const size_t kMin = (size_t)4 << 20;
    int parts = total >= kMin ? (int)(total / (kMin / 2)) : 1;
    if (parts > kThreads) parts = kThreads;
    if (parts < 2 || n < 2) {
        CopyJob j = {dst, src, len, 0, n};
        copy_job(&j);
        return;
    }
    CopyJob jobs[kThreads];
    pthread_t th[kThreads];
    int started[kThreads] = {0};
    size_t i = 0, acc = 0;
    for (int t = 0; t < parts; ++t) {
        const size_t goal = total / parts * (size_t)(t + 1);
        jobs[t].dst = dst;
        jobs[t].src = src;
        jobs[t].len = len;
        jobs[t].b = i;
        while (i < n && (acc < goal || t == parts - 1)) acc += len[i++];
        jobs[t].e = i;
    }
    for (int t = 1; t < parts; ++t) started[t] = pthread_create(&th[t], NULL, copy_job, &jobs[t]) == 0;
    copy_job(&jobs[0]);
    for (int t = 1; t < parts; ++t) {
        if (started[t]) pthread_join(th[t], NULL);
        else copy_job(&jobs[t]);
    }
}

/* ------------------------------------------------------------ key slot -- */

/* A single-slot device key table, created on first use.  The slot is
 * read-only after creation, so objects may be used from any thread.
 * First use cannot create it twice for one object: every caller of
 * oneslot_ready holds the GIL, and nothing between the NULL test and the
 * point where kt holds a table with its key installed releases it -- session(),
 * qpp_keytab_create and qpp_session_set_keys are plain C calls into the
 * library (none is wrapped in Py_BEGIN_ALLOW_THREADS, none calls back into
 * Python), so a second thread's first use starts after the first one's has
 * ended and finds kt set.  The extension is built for the limited API, which
 * a free-threaded interpreter does not load. */
typedef struct {
    qpp_key_material km;
    qpp_keytab *kt;
} OneSlot;

static int oneslot_ready(OneSlot *o)
{
    if (o->kt) return 0;
    qpp_session *s = session();
    if (!s) return -1;
    int rc = qpp_keytab_create(1, &o->kt);
    if (rc == QPP_OK) rc = qpp_session_set_keys(s, o->kt, &o->km, 1);
    if (rc != QPP_OK) {
        if (o->kt) qpp_keytab_destroy(o->kt);
        o->kt = NULL;
        return check_rc(rc);
    }
    return 0;
}

static void oneslot_reset(OneSlot *o, int suite)
{
    if (o->kt) qpp_keytab_destroy(o->kt);
    o->kt = NULL;
    memset(&o->km, 0, sizeof(o->km));
    o->km.suite = (uint8_t)suite;
}

/* ---------------------------------------------------------------- AEAD -- */

typedef struct {
    PyObject_HEAD
    OneSlot s;
} AEADObject;

/* The constructor's argument checks and the key material, without the device
 * table: AEAD(...) creates that at once, aead_deferred(...) at first use. */
static int aead_fill(AEADObject *self, PyObject *args)
{
    const char *name;
    const unsigned char *key, *iv;
    Py_ssize_t name_len, key_len, iv_len;
    if (!PyArg_ParseTuple(args, "y#y#y#", &name, &name_len, &key, &key_len, &iv, &iv_len))
        return -1;
    int suite = aead_suite(name, name_len);
    if (suite < 0) {
        PyErr_Format(g_crypto_error, "Invalid cipher name: %s", name);
        return -1;
    }
    if (key_len > 32) {
        PyErr_SetString(g_crypto_error, "Invalid key length");
        return -1;
    }
    if (iv_len > 12) {
        PyErr_SetString(g_crypto_error, "Invalid iv length");
        return -1;
    }
    if (key_len != suite_key_len(suite)) {
        /* the reference fails in EVP_CIPHER_CTX_set_key_length */
        PyErr_SetString(g_crypto_error, "OpenSSL call failed");
        return -1;
    }
    oneslot_reset(&self->s, suite);
    memcpy(self->s.km.key, key, (size_t)key_len);
    memcpy(self->s.km.iv, iv, (size_t)iv_len); /* short iv: zero padded, as the reference */
    return 0;
}

static int AEAD_init(AEADObject *self, PyObject *args, PyObject *kwargs)
{
    if (aead_fill(self, args) < 0) return -1;
    return oneslot_ready(&self->s);
}

/* aead_deferred(cipher_name, key, iv) -> an AEAD whose one-slot device table
 * is created by its first encrypt / decrypt (aead_run's oneslot_ready), not
 * here: the batched key-update path builds one per connection and most are
 * only ever read through _material().  The same argument checks and errors as
 * AEAD(...); without a device the RuntimeError comes at first use instead. */
static PyObject *py_aead_deferred(PyObject *m, PyObject *args)
{
    allocfunc alloc = (allocfunc)PyType_GetSlot((PyTypeObject *)g_aead_type, Py_tp_alloc);
    AEADObject *self = (AEADObject *)alloc((PyTypeObject *)g_aead_type, 0);  /* zeroed: s.kt NULL */
    if (!self) return NULL;
    if (aead_fill(self, args) < 0) {
        Py_DECREF(self);
        return NULL;
    }
    return (PyObject *)self;
}

static void AEAD_dealloc(AEADObject *self)
{
    if (self->s.kt) qpp_keytab_destroy(self->s.kt);
    heap_dealloc((PyObject *)self);
}

/* in = aad || data; AEAD only (QPP_F_NO_HP) */
static PyObject *aead_run(AEADObject *self, PyObject *args, int enc)
{
    const unsigned char *data, *aad;
    Py_ssize_t data_len, aad_len;
    unsigned long long pn;
    if (!PyArg_ParseTuple(args, "y#y#K", &data, &data_len, &aad, &aad_len, &pn)) return NULL;
    if ((enc ? 0 : data_len < QPP_TAG_LEN) || data_len > QPP_PACKET_MAX || aad_len > QPP_MAX_HDR) {
        PyErr_SetString(g_crypto_error, "Invalid payload length");
        return NULL;
    }
    if (oneslot_ready(&self->s) < 0) return NULL;
    qpp_session *s = session();
    if (!s) return NULL;
    size_t in_len = (size_t)(aad_len + data_len);
    size_t out_len = in_len + (enc ? QPP_TAG_LEN : 0);
    unsigned char *buf = PyMem_Malloc(in_len + out_len + 1);
    if (!buf) return PyErr_NoMemory();
    memcpy(buf, aad, (size_t)aad_len);
    memcpy(buf + aad_len, data, (size_t)data_len);
    qpp_desc d;
    memset(&d, 0, sizeof d);
    d.len = (uint32_t)(enc ? data_len : aad_len + data_len);
    d.hdr_len = (uint16_t)aad_len;
    d.flags = QPP_F_NO_HP;
    d.pn = pn;
    qpp_result r;
    int rc = enc ? qpp_session_protect(s, self->s.kt, &d, 1, buf, in_len, buf + in_len, out_len, &r)
                 : qpp_session_unprotect(s, self->s.kt, &d, 1, buf, in_len, buf + in_len, out_len, &r);
    PyObject *ret = NULL;
    if (check_rc(rc) == 0) {
        if (r.status == QPP_S_OK)
            ret = PyBytes_FromStringAndSize((const char *)buf + in_len + aad_len,
                                            enc ? data_len + QPP_TAG_LEN : data_len - QPP_TAG_LEN);
        else if (r.status == QPP_S_DECRYPT)
            PyErr_SetString(g_crypto_error, "Payload decryption failed");
        else if (r.status == QPP_S_INTERNAL)
            PyErr_SetString(g_crypto_error, "Internal error: the packet was not processed");
        else
            PyErr_SetString(g_crypto_error, "Invalid payload length");
    }
    PyMem_Free(buf);
    return ret;
}

static PyObject *AEAD_encrypt(AEADObject *self, PyObject *args) { return aead_run(self, args, 1); }
static PyObject *AEAD_decrypt(AEADObject *self, PyObject *args) { return aead_run(self, args, 0); }

/* (suite, key, iv): lets the packet-level wrapper build fused key slots */
static PyObject *AEAD_material(AEADObject *self, PyObject *unused)
{
    int kl = suite_key_len(self->s.km.suite);
    return Py_BuildValue("iy#y#", (int)self->s.km.suite, self->s.km.key, (Py_ssize_t)kl,
                         self->s.km.iv, (Py_ssize_t)12);
}

static PyMethodDef AEAD_methods[] = {
    {"encrypt", (PyCFunction)AEAD_encrypt, METH_VARARGS, "encrypt(data, associated_data, packet_number) -> bytes"},
    {"decrypt", (PyCFunction)AEAD_decrypt, METH_VARARGS, "decrypt(data, associated_data, packet_number) -> bytes"},
    {"_material", (PyCFunction)AEAD_material, METH_NOARGS, "(suite, key, iv)"},
    {NULL},
};

static PyType_Slot AEAD_slots[] = {
    {Py_tp_doc, "AEAD payload protection on the GPU"},
    {Py_tp_methods, AEAD_methods},
    {Py_tp_init, AEAD_init},
    {Py_tp_new, PyType_GenericNew},
    {Py_tp_dealloc, AEAD_dealloc},
    {0, NULL},
};

static PyType_Spec AEAD_spec = {"aioquic_amd._crypto.AEAD", sizeof(AEADObject), 0,
                                Py_TPFLAGS_DEFAULT, AEAD_slots};

/* ---------------------------------------------------- HeaderProtection -- */

typedef struct {
    PyObject_HEAD
    OneSlot s;
} HPObject;

static int HP_init(HPObject *self, PyObject *args, PyObject *kwargs)
{
    const char *name;
    const unsigned char *key;
    Py_ssize_t name_len, key_len;
    if (!PyArg_ParseTuple(args, "y#y#", &name, &name_len, &key, &key_len)) return -1;
    int suite = hp_suite(name, name_len);
    if (suite < 0) {
        PyErr_Format(g_crypto_error, "Invalid cipher name: %s", name);
        return -1;
    }
    if (key_len != suite_key_len(suite)) {
        PyErr_SetString(g_crypto_error, "OpenSSL call failed");
        return -1;
    }
    oneslot_reset(&self->s, suite);
    memcpy(self->s.km.hp, key, (size_t)key_len);
    return oneslot_ready(&self->s);
}

static void HP_dealloc(HPObject *self)
{
    if (self->s.kt) qpp_keytab_destroy(self->s.kt);
    heap_dealloc((PyObject *)self);
}

static int hp_mask(HPObject *self, const unsigned char *sample, unsigned char mask[16])
{
    if (oneslot_ready(&self->s) < 0) return -1;
    qpp_session *s = session();
    if (!s) return -1;
    uint32_t slot = 0;
    return check_rc(qpp_session_hp_mask(s, self->s.kt, &slot, sample, 1, mask));
}

static unsigned char first_byte_bits(unsigned char b0) { return (b0 & 0x80) ? 0x0f : 0x1f; }

/* HeaderProtection.apply (_crypto.c:289-319) */
static PyObject *HP_apply(HPObject *self, PyObject *args)
{
    const unsigned char *hdr, *payload;
    Py_ssize_t hlen, plen;
    if (!PyArg_ParseTuple(args, "y#y#", &hdr, &hlen, &payload, &plen)) return NULL;
    if (hlen < 1) {
        PyErr_SetString(g_crypto_error, "Invalid payload length");
        return NULL;
    }
    int pn_len = (hdr[0] & 3) + 1;
    Py_ssize_t pn_off = hlen - pn_len;
    /* hlen + plen > 1500 overruns the reference's buffer (_crypto.c:305-306) */
    if (pn_off < 0 || plen < 20 - pn_len || hlen + plen > QPP_PACKET_MAX) {
        PyErr_SetString(g_crypto_error, "Invalid payload length");
        return NULL;
    }
    unsigned char mask[16];
    if (hp_mask(self, payload + 4 - pn_len, mask) < 0) return NULL;
    PyObject *out = PyBytes_FromStringAndSize(NULL, hlen + plen);
    if (!out) return NULL;
    unsigned char *o = (unsigned char *)PyBytes_AsString(out);
    memcpy(o, hdr, (size_t)hlen);
    memcpy(o + hlen, payload, (size_t)plen);
    o[0] ^= mask[0] & first_byte_bits(o[0]);
    for (int i = 0; i < pn_len; ++i) o[pn_off + i] ^= mask[1 + i];
    return out;
}

/* HeaderProtection.remove (_crypto.c:321-350): returns (header, truncated pn as C int) */
static PyObject *HP_remove(HPObject *self, PyObject *args)
{
    const unsigned char *pkt;
    Py_ssize_t len;
    unsigned int pn_off;
    if (!PyArg_ParseTuple(args, "y#I", &pkt, &len, &pn_off)) return NULL;
    if ((Py_ssize_t)pn_off + 20 > len) {
        PyErr_SetString(g_crypto_error, "Invalid payload length");
        return NULL;
    }
    unsigned char mask[16];
    if (hp_mask(self, pkt + pn_off + 4, mask) < 0) return NULL;
    unsigned char *buf = PyMem_Malloc((size_t)pn_off + 4);
    if (!buf) return PyErr_NoMemory();
    memcpy(buf, pkt, (size_t)pn_off + 4);
    buf[0] ^= mask[0] & first_byte_bits(buf[0]);
    int pn_len = (buf[0] & 3) + 1;
    uint32_t trunc = 0;
    for (int i = 0; i < pn_len; ++i) {
        buf[pn_off + i] ^= mask[1 + i];
        trunc = (trunc << 8) | buf[pn_off + i];
    }
    PyObject *ret = Py_BuildValue("y#i", buf, (Py_ssize_t)(pn_off + pn_len), (int)trunc);
    PyMem_Free(buf);
    return ret;
}

static PyObject *HP_material(HPObject *self, PyObject *unused)
{
    return Py_BuildValue("iy#", (int)self->s.km.suite, self->s.km.hp,
                         (Py_ssize_t)suite_key_len(self->s.km.suite));
}

static PyMethodDef HP_methods[] = {
    {"apply", (PyCFunction)HP_apply, METH_VARARGS, "apply(plain_header, protected_payload) -> bytes"},
    {"remove", (PyCFunction)HP_remove, METH_VARARGS, "remove(packet, encrypted_offset) -> (bytes, int)"},
    {"_material", (PyCFunction)HP_material, METH_NOARGS, "(suite, key)"},
    {NULL},
};

static PyType_Slot HP_slots[] = {
    {Py_tp_doc, "QUIC header protection masks on the GPU"},
    {Py_tp_methods, HP_methods},
    {Py_tp_init, HP_init},
    {Py_tp_new, PyType_GenericNew},
    {Py_tp_dealloc, HP_dealloc},
    {0, NULL},
};

static PyType_Spec HP_spec = {"aioquic_amd._crypto.HeaderProtection", sizeof(HPObject), 0,
                              Py_TPFLAGS_DEFAULT, HP_slots};

/* ------------------------------------------------------------ KeyTable -- */

typedef struct {
    PyObject_HEAD
    qpp_keytab *kt;
} KeyTableObject;

static int KT_init(KeyTableObject *self, PyObject *args, PyObject *kwargs)
{
    unsigned int cap;
    if (!PyArg_ParseTuple(args, "I", &cap)) return -1;
    if (self->kt) {
        qpp_keytab_destroy(self->kt);
        self->kt = NULL;
    }
    int rc = qpp_keytab_create(cap, &self->kt);
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "invalid key-table capacity");
        return -1;
    }
    return check_rc(rc);
}

static void KT_dealloc(KeyTableObject *self)
{
    if (self->kt) qpp_keytab_destroy(self->kt);
    heap_dealloc((PyObject *)self);
}

/* set(materials: bytes-like of n packed qpp_key_material records, stream=0) */
static PyObject *KT_set(KeyTableObject *self, PyObject *args)
{
    const char *b;
    Py_ssize_t len;
    unsigned long long stream = 0;
    if (!PyArg_ParseTuple(args, "y#|K", &b, &len, &stream)) return NULL;
    if (len % (Py_ssize_t)sizeof(qpp_key_material)) {
        PyErr_SetString(PyExc_ValueError, "materials must be a whole number of 84-byte records");
        return NULL;
    }
    uint32_t n = (uint32_t)(len / (Py_ssize_t)sizeof(qpp_key_material));
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = qpp_keytab_set(self->kt, (const qpp_key_material *)b, n, as_ptr(stream));
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad key material (slot out of range or unknown suite)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

/* KeyTable.derive(secrets) -> key material: batched CryptoContext.setup
 * (qpp_keytab_derive); secrets = whole qpp_secret records. */
static PyObject *KT_derive(KeyTableObject *self, PyObject *args)
{
    const char *b;
    Py_ssize_t len;
    unsigned long long stream = 0;
    if (!PyArg_ParseTuple(args, "y#|K", &b, &len, &stream)) return NULL;
    if (len % (Py_ssize_t)sizeof(qpp_secret)) {
        PyErr_SetString(PyExc_ValueError, "secrets must be a whole number of 80-byte records");
        return NULL;
    }
    uint32_t n = (uint32_t)(len / (Py_ssize_t)sizeof(qpp_secret));
    PyObject *km = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)n * (Py_ssize_t)sizeof(qpp_key_material));
    if (!km) return NULL;
    qpp_key_material *out = (qpp_key_material *)PyBytes_AsString(km);
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = qpp_keytab_derive(self->kt, (const qpp_secret *)b, n, out, as_ptr(stream));
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG) {
        Py_DECREF(km);
        PyErr_SetString(PyExc_ValueError, "bad secret (slot out of range, unknown suite or length)");
        return NULL;
    }
    if (check_rc(rc) < 0) {
        Py_DECREF(km);
        return NULL;
    }
    return km;
}

/* KeyTable.derive_initial(records[, stream]) -> (key material, secrets):
 * batched CryptoPair.setup_initial (qpp_keytab_derive_initial); records = whole
 * qpp_initial records; two qpp_key_material and two 32-byte secrets per record. */
static PyObject *KT_derive_initial(KeyTableObject *self, PyObject *args)
{
    const char *b;
    Py_ssize_t len;
    unsigned long long stream = 0;
    if (!PyArg_ParseTuple(args, "y#|K", &b, &len, &stream)) return NULL;
    if (len % (Py_ssize_t)sizeof(qpp_initial) || len / (Py_ssize_t)sizeof(qpp_initial) > (1 << 24)) {
        PyErr_SetString(PyExc_ValueError, "records must be a whole number (up to 2^24) of 32-byte records");
        return NULL;
    }
    uint32_t n = (uint32_t)(len / (Py_ssize_t)sizeof(qpp_initial));
    PyObject *km = PyBytes_FromStringAndSize(NULL, 2 * (Py_ssize_t)n * (Py_ssize_t)sizeof(qpp_key_material));
    PyObject *sec = PyBytes_FromStringAndSize(NULL, 2 * (Py_ssize_t)n * 32);
    if (!km || !sec) {
        Py_XDECREF(km);
        Py_XDECREF(sec);
        return NULL;
    }
    qpp_key_material *out = (qpp_key_material *)PyBytes_AsString(km);
    uint8_t *sout = (uint8_t *)PyBytes_AsString(sec);
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = qpp_keytab_derive_initial(self->kt, (const qpp_initial *)b, n, out, sout, as_ptr(stream));
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG)
        PyErr_SetString(PyExc_ValueError,
                        "bad initial record (slot out of range or used twice, cid longer than 20, unknown flag)");
    if (rc == QPP_E_ARG || check_rc(rc) < 0) {
        Py_DECREF(km);
        Py_DECREF(sec);
        return NULL;
    }
    PyObject *ret = PyTuple_Pack(2, km, sec);
    Py_DECREF(km);
    Py_DECREF(sec);
    return ret;
}

/* KeyTable.derive_next(records[, stream]) -> (key material, secrets): batched
 * next_key_phase (qpp_keytab_derive_next); records = whole qpp_next_phase
 * records; one qpp_key_material and one 64-byte zero-padded secret per record. */
static PyObject *KT_derive_next(KeyTableObject *self, PyObject *args)
{
    const char *b;
    Py_ssize_t len;
    unsigned long long stream = 0;
    if (!PyArg_ParseTuple(args, "y#|K", &b, &len, &stream)) return NULL;
    if (len % (Py_ssize_t)sizeof(qpp_next_phase) || len / (Py_ssize_t)sizeof(qpp_next_phase) > (1 << 24)) {
        PyErr_SetString(PyExc_ValueError, "records must be a whole number (up to 2^24) of 104-byte records");
        return NULL;
    }
    uint32_t n = (uint32_t)(len / (Py_ssize_t)sizeof(qpp_next_phase));
    PyObject *km = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)n * (Py_ssize_t)sizeof(qpp_key_material));
    PyObject *sec = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)n * 64);
    if (!km || !sec) {
        Py_XDECREF(km);
        Py_XDECREF(sec);
        return NULL;
    }
    qpp_key_material *out = (qpp_key_material *)PyBytes_AsString(km);
    uint8_t *sout = (uint8_t *)PyBytes_AsString(sec);
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = qpp_keytab_derive_next(self->kt, (const qpp_next_phase *)b, n, out, sout, as_ptr(stream));
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG)
        PyErr_SetString(PyExc_ValueError,
                        "bad next-phase record (slot out of range, unknown suite, secret length, key phase or flag)");
    if (rc == QPP_E_ARG || check_rc(rc) < 0) {
        Py_DECREF(km);
        Py_DECREF(sec);
        return NULL;
    }
    PyObject *ret = PyTuple_Pack(2, km, sec);
    Py_DECREF(km);
    Py_DECREF(sec);
    return ret;
}

/* KeyTable.derive_trace(enable=-1) -> (derive_ms, setup_ms) of the last timed
 * derive_initial or derive_next call (qpp_keytab_derive_trace). */
static PyObject *KT_derive_trace(KeyTableObject *self, PyObject *args)
{
    int enable = -1;
    if (!PyArg_ParseTuple(args, "|i", &enable)) return NULL;
    float d = 0, k = 0;
    if (check_rc(qpp_keytab_derive_trace(self->kt, enable, &d, &k)) < 0) return NULL;
    return Py_BuildValue("dd", (double)d, (double)k);
}

static PyObject *KT_clear(KeyTableObject *self, PyObject *args)
{
    const char *b;
    Py_ssize_t len;
    if (!PyArg_ParseTuple(args, "y#", &b, &len)) return NULL;
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = qpp_keytab_clear(self->kt, (const uint32_t *)b, (uint32_t)(len / 4), NULL);
    Py_END_ALLOW_THREADS
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *KT_capacity(KeyTableObject *self, void *unused)
{
    return PyLong_FromUnsignedLong(qpp_keytab_capacity(self->kt));
}

static PyMethodDef KT_methods[] = {
    {"set", (PyCFunction)KT_set, METH_VARARGS, "set(materials, stream=0)"},
    {"clear", (PyCFunction)KT_clear, METH_VARARGS, "clear(slots_u32)"},
    {"derive", (PyCFunction)KT_derive, METH_VARARGS, "derive(secrets, stream=0) -> key material"},
    {"derive_initial", (PyCFunction)KT_derive_initial, METH_VARARGS,
     "derive_initial(records, stream=0) -> (key material, secrets)"},
    {"derive_next", (PyCFunction)KT_derive_next, METH_VARARGS,
     "derive_next(records, stream=0) -> (key material, secrets)"},
    {"derive_trace", (PyCFunction)KT_derive_trace, METH_VARARGS,
     "derive_trace(enable=-1) -> (derive_ms, setup_ms) of the last timed derive_initial / derive_next"},
    {NULL},
};

static PyGetSetDef KT_getset[] = {
    {"capacity", (getter)KT_capacity, NULL, "number of key slots", NULL},
    {NULL},
};

static PyType_Slot KT_slots[] = {
    {Py_tp_doc, "device-resident expanded key slots"},
    {Py_tp_methods, KT_methods},
    {Py_tp_getset, KT_getset},
    {Py_tp_init, KT_init},
    {Py_tp_new, PyType_GenericNew},
    {Py_tp_dealloc, KT_dealloc},
    {0, NULL},
};

static PyType_Spec KT_spec = {"aioquic_amd._crypto.KeyTable", sizeof(KeyTableObject), 0,
                              Py_TPFLAGS_DEFAULT, KT_slots};

static qpp_keytab *as_table(PyObject *o)
{
    if (!PyObject_TypeCheck(o, (PyTypeObject *)g_kt_type)) {
        PyErr_SetString(PyExc_TypeError, "expected a KeyTable");
        return NULL;
    }
    return ((KeyTableObject *)o)->kt;
}

/* ---------------------------------------------------------------- Plan -- */

typedef struct {
    PyObject_HEAD
    qpp_plan *plan;
} PlanObject;

static int Plan_init(PlanObject *self, PyObject *args, PyObject *kwargs)
{
    unsigned int cap;
    if (!PyArg_ParseTuple(args, "I", &cap)) return -1;
    if (self->plan) {
        qpp_plan_destroy(self->plan);
        self->plan = NULL;
    }
    int rc = qpp_plan_create(cap, &self->plan);
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "invalid plan capacity");
        return -1;
    }
    return check_rc(rc);
}

static void Plan_dealloc(PlanObject *self)
{
    if (self->plan) qpp_plan_destroy(self->plan);
    heap_dealloc((PyObject *)self);
}

static PyType_Slot Plan_slots[] = {
    {Py_tp_doc, "device scratch of the (suite, key slot) bucketing step"},
    {Py_tp_init, Plan_init},
    {Py_tp_new, PyType_GenericNew},
    {Py_tp_dealloc, Plan_dealloc},
    {0, NULL},
};

static PyType_Spec Plan_spec = {"aioquic_amd._crypto.Plan", sizeof(PlanObject), 0,
                                Py_TPFLAGS_DEFAULT, Plan_slots};

/* NULL for None, else the plan (NULL with an exception set for a wrong type) */
static int as_plan(PyObject *o, qpp_plan **out)
{
    *out = NULL;
    if (!o || o == Py_None) return 0;
    if (!PyObject_TypeCheck(o, (PyTypeObject *)g_plan_type)) {
        PyErr_SetString(PyExc_TypeError, "expected a Plan or None");
        return -1;
    }
    *out = ((PlanObject *)o)->plan;
    return 0;
}

/* -------------------------------------------------------------- CidMap -- */

/* CidMap(capacity): the device-resident connection-ID map of qpp_route
 * (qpp_cidmap, quic_pp.h).  Records are packed 32-byte qpp_cid_entry. */
typedef struct {
    PyObject_HEAD
    qpp_cidmap *map;
} CidMapObject;

static int CidMap_init(CidMapObject *self, PyObject *args, PyObject *kwargs)
{
    unsigned int cap;
    if (!PyArg_ParseTuple(args, "I", &cap)) return -1;
    if (self->map) {
        qpp_cidmap_destroy(self->map);
        self->map = NULL;
    }
    int rc = qpp_cidmap_create(cap, &self->map);
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "invalid connection-ID map capacity");
        return -1;
    }
    return check_rc(rc);
}

static void CidMap_dealloc(CidMapObject *self)
{
    if (self->map) qpp_cidmap_destroy(self->map);
    heap_dealloc((PyObject *)self);
}

static PyObject *cidmap_change(CidMapObject *self, PyObject *args, int put)
{
    const char *b;
    Py_ssize_t len;
    unsigned long long stream = 0;
    if (!PyArg_ParseTuple(args, "y#|K", &b, &len, &stream)) return NULL;
    if (len % (Py_ssize_t)sizeof(qpp_cid_entry)) {
        PyErr_SetString(PyExc_ValueError, "records must be a whole number of 32-byte entries");
        return NULL;
    }
    const uint32_t n = (uint32_t)(len / (Py_ssize_t)sizeof(qpp_cid_entry));
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = (put ? qpp_cidmap_put : qpp_cidmap_remove)(self->map, (const qpp_cid_entry *)b, n, as_ptr(stream));
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, put ? "bad entries (a CID length outside 1..20, or more CIDs than the "
                                                "map's capacity); nothing was changed"
                                              : "bad entries (a CID length outside 1..20); nothing was changed");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *CidMap_put(CidMapObject *self, PyObject *args) { return cidmap_change(self, args, 1); }
static PyObject *CidMap_remove(CidMapObject *self, PyObject *args) { return cidmap_change(self, args, 0); }

static PyObject *cidmap_query(CidMapObject *self, PyObject *args, int home)
{
    const char *cid;
    Py_ssize_t len;
    if (!PyArg_ParseTuple(args, "y#", &cid, &len)) return NULL;
    if (len < 1 || len > QPP_CID_MAX) {
        PyErr_SetString(PyExc_ValueError, "connection ID must be 1..20 bytes");
        return NULL;
    }
    const uint32_t v = (home ? qpp_cidmap_home : qpp_cidmap_find)(self->map, (const uint8_t *)cid, (uint32_t)len);
    if (!home && v == QPP_CONN_NONE) Py_RETURN_NONE;
    return PyLong_FromUnsignedLong(v);
}

static PyObject *CidMap_find(CidMapObject *self, PyObject *args) { return cidmap_query(self, args, 0); }
static PyObject *CidMap_home(CidMapObject *self, PyObject *args) { return cidmap_query(self, args, 1); }
static PyObject *CidMap_count(CidMapObject *self, void *unused) { return PyLong_FromUnsignedLong(qpp_cidmap_count(self->map)); }
static PyObject *CidMap_buckets(CidMapObject *self, void *unused) { return PyLong_FromUnsignedLong(qpp_cidmap_buckets(self->map)); }

static PyMethodDef CidMap_methods[] = {
    {"put", (PyCFunction)CidMap_put, METH_VARARGS, "put(records, stream=0): add CIDs or replace their connection"},
    {"remove", (PyCFunction)CidMap_remove, METH_VARARGS, "remove(records, stream=0): retire CIDs (absent ones are ignored)"},
    {"find", (PyCFunction)CidMap_find, METH_VARARGS, "find(cid) -> connection index or None (the host mirror)"},
    {"home", (PyCFunction)CidMap_home, METH_VARARGS, "home(cid) -> the CID's home bucket (diagnostic)"},
    {NULL},
};

static PyGetSetDef CidMap_getset[] = {
    {"count", (getter)CidMap_count, NULL, "CIDs in the map", NULL},
    {"buckets", (getter)CidMap_buckets, NULL, "buckets of the table", NULL},
    {NULL},
};

static PyType_Slot CidMap_slots[] = {
    {Py_tp_doc, "device-resident connection-ID map"},
    {Py_tp_methods, CidMap_methods},
    {Py_tp_getset, CidMap_getset},
    {Py_tp_init, CidMap_init},
    {Py_tp_new, PyType_GenericNew},
    {Py_tp_dealloc, CidMap_dealloc},
    {0, NULL},
};

static PyType_Spec CidMap_spec = {"aioquic_amd._crypto.CidMap", sizeof(CidMapObject), 0,
                                  Py_TPFLAGS_DEFAULT, CidMap_slots};

static qpp_cidmap *as_cidmap(PyObject *o)
{
    if (!PyObject_TypeCheck(o, (PyTypeObject *)g_cidmap_type)) {
        PyErr_SetString(PyExc_TypeError, "expected a CidMap");
        return NULL;
    }
    return ((CidMapObject *)o)->map;
}

/* --------------------------------------------------------- MultiSession -- */

/* MultiSession(devices, key_capacity): one host batch over several GPUs
 * (qpp_multi, quic_pp.h).  .set_keys(materials), .protect(desc, data,
 * out_len) / .unprotect(...) -> (out, results) like protect_host; .devices. */
typedef struct {
    PyObject_HEAD
    qpp_multi *m;
} MultiObject;

static int Multi_init(MultiObject *self, PyObject *args, PyObject *kwargs)
{
    PyObject *devs;
    unsigned int cap;
    if (!PyArg_ParseTuple(args, "OI", &devs, &cap)) return -1;
    const Py_ssize_t nd = PySequence_Size(devs);
    int ids[16];
    if (nd < 0) return -1;
    if (nd < 1 || nd > 16) {
        PyErr_SetString(PyExc_ValueError, "1 to 16 devices");
        return -1;
    }
    for (Py_ssize_t k = 0; k < nd; ++k) {
        PyObject *it = PySequence_GetItem(devs, k);
        if (!it) return -1;
        ids[k] = (int)PyLong_AsLong(it);
        Py_DECREF(it);
        if (ids[k] == -1 && PyErr_Occurred()) return -1;
    }
    if (self->m) {
        qpp_multi_destroy(self->m);
        self->m = NULL;
    }
    int rc = qpp_multi_create(ids, (int)nd, cap, &self->m);
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad device list or key capacity");
        return -1;
    }
    return check_rc(rc);
}

static void Multi_dealloc(MultiObject *self)
{
    if (self->m) qpp_multi_destroy(self->m);
    heap_dealloc((PyObject *)self);
}

static PyObject *Multi_set_keys(MultiObject *self, PyObject *args)
{
    const char *b;
    Py_ssize_t len;
    if (!PyArg_ParseTuple(args, "y#", &b, &len)) return NULL;
    if (len % (Py_ssize_t)sizeof(qpp_key_material)) {
        PyErr_SetString(PyExc_ValueError, "materials must be a whole number of 84-byte records");
        return NULL;
    }
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = qpp_multi_set_keys(self->m, (const qpp_key_material *)b, (uint32_t)(len / (Py_ssize_t)sizeof(qpp_key_material)));
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad key material (slot out of range or unknown suite)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *multi_run_py(MultiObject *self, PyObject *args, int enc)
{
    const char *desc, *data;
    Py_ssize_t desc_len, data_len, out_len;
    if (!PyArg_ParseTuple(args, "y#y#n", &desc, &desc_len, &data, &data_len, &out_len)) return NULL;
    if (desc_len % (Py_ssize_t)sizeof(qpp_desc) || out_len < 0) {
        PyErr_SetString(PyExc_ValueError, "bad descriptor buffer or output length");
        return NULL;
    }
    const uint32_t n = (uint32_t)(desc_len / (Py_ssize_t)sizeof(qpp_desc));
    PyObject *out = PyBytes_FromStringAndSize(NULL, out_len);
    PyObject *res = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)n * (Py_ssize_t)sizeof(qpp_result));
    PyObject *ret = NULL;
    if (out && res) {
        int rc;
        char *o = PyBytes_AsString(out), *r = PyBytes_AsString(res);
        Py_BEGIN_ALLOW_THREADS
        rc = enc ? qpp_multi_protect(self->m, (const qpp_desc *)desc, n, (const uint8_t *)data, (size_t)data_len,
                                     (uint8_t *)o, (size_t)out_len, (qpp_result *)r)
                 : qpp_multi_unprotect(self->m, (const qpp_desc *)desc, n, (const uint8_t *)data, (size_t)data_len,
                                       (uint8_t *)o, (size_t)out_len, (qpp_result *)r);
        Py_END_ALLOW_THREADS
        if (check_rc(rc) == 0) ret = PyTuple_Pack(2, out, res);
    }
    Py_XDECREF(out);
    Py_XDECREF(res);
    return ret;
}

static PyObject *Multi_protect(MultiObject *self, PyObject *args) { return multi_run_py(self, args, 1); }
static PyObject *Multi_unprotect(MultiObject *self, PyObject *args) { return multi_run_py(self, args, 0); }

/* protect_into / unprotect_into(desc_ptr, n, in_ptr, in_len, out_ptr, out_len,
 * res_ptr): host memory by address (caller-owned, reused across batches). */
static PyObject *multi_into_py(MultiObject *self, PyObject *args, int enc)
{
    unsigned long long dp, ip, op, rp, in_len, out_len;
    unsigned int n;
    if (!PyArg_ParseTuple(args, "KIKKKKK", &dp, &n, &ip, &in_len, &op, &out_len, &rp)) return NULL;
    if (n && (!dp || !rp || (in_len && !ip) || (out_len && !op))) {
        PyErr_SetString(PyExc_ValueError, "null buffer");
        return NULL;
    }
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = enc ? qpp_multi_protect(self->m, (const qpp_desc *)as_ptr(dp), n, (const uint8_t *)as_ptr(ip),
                                 (size_t)in_len, (uint8_t *)as_ptr(op), (size_t)out_len, (qpp_result *)as_ptr(rp))
             : qpp_multi_unprotect(self->m, (const qpp_desc *)as_ptr(dp), n, (const uint8_t *)as_ptr(ip),
                                   (size_t)in_len, (uint8_t *)as_ptr(op), (size_t)out_len, (qpp_result *)as_ptr(rp));
    Py_END_ALLOW_THREADS
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *Multi_protect_into(MultiObject *self, PyObject *args) { return multi_into_py(self, args, 1); }
static PyObject *Multi_unprotect_into(MultiObject *self, PyObject *args) { return multi_into_py(self, args, 0); }

/* trace(enable=-1) -> [dict per device]: the phases of each device session's
 * last traced pipelined call (qpp_multi_trace); enable 1 / 0 turns tracing
 * on / off for the following calls. */
static PyObject *Multi_trace(MultiObject *self, PyObject *args)
{
    int enable = -1;
    if (!PyArg_ParseTuple(args, "|i", &enable)) return NULL;
    qpp_trace t[16];
    const int k = qpp_multi_trace(self->m, enable, t, 16);
    if (k < 0) {
        check_rc(k);
        return NULL;
    }
    PyObject *lst = PyList_New(0);
    for (int i = 0; lst && i < k; ++i) {
        PyObject *d = Py_BuildValue(
            "{s:I,s:I,s:d,s:d,s:d,s:d,s:d,s:d,s:d,s:d,s:d,s:d,s:d}", "pipelined", t[i].pipelined, "chunks",
            t[i].chunks, "total_ms", t[i].total_ms, "submit_ms", t[i].submit_ms, "copy_in_ms", t[i].copy_in_ms,
            "copy_out_ms", t[i].copy_out_ms, "wait_ms", t[i].wait_ms, "h2d_ms", t[i].h2d_ms, "kernel_ms",
            t[i].kernel_ms, "d2h_ms", t[i].d2h_ms, "gpu_span_ms", t[i].gpu_span_ms, "in_bytes", t[i].in_bytes,
            "out_bytes", t[i].out_bytes);
        if (!d || PyList_Append(lst, d) < 0) {
            Py_XDECREF(d);
            Py_DECREF(lst);
            return NULL;
        }
        Py_DECREF(d);
    }
    return lst;
}

static PyObject *Multi_devices(MultiObject *self, void *unused)
{
    return PyLong_FromLong(qpp_multi_devices(self->m));
}

static PyMethodDef Multi_methods[] = {
    {"set_keys", (PyCFunction)Multi_set_keys, METH_VARARGS, "set_keys(materials) on every device"},
    {"protect", (PyCFunction)Multi_protect, METH_VARARGS, "protect(desc, data, out_len) -> (out, results)"},
    {"unprotect", (PyCFunction)Multi_unprotect, METH_VARARGS, "unprotect(desc, data, out_len) -> (out, results)"},
    {"protect_into", (PyCFunction)Multi_protect_into, METH_VARARGS,
     "protect_into(desc_ptr, n, in_ptr, in_len, out_ptr, out_len, res_ptr)"},
    {"unprotect_into", (PyCFunction)Multi_unprotect_into, METH_VARARGS,
     "unprotect_into(desc_ptr, n, in_ptr, in_len, out_ptr, out_len, res_ptr)"},
    {"trace", (PyCFunction)Multi_trace, METH_VARARGS,
     "trace(enable=-1) -> per device, the last traced call's host / PCIe / kernel phases"},
    {NULL},
};

static PyGetSetDef Multi_getset[] = {
    {"devices", (getter)Multi_devices, NULL, "number of device sessions", NULL},
    {NULL},
};

static PyType_Slot Multi_slots[] = {
    {Py_tp_doc, "one host batch over several GPUs (qpp_multi)"},
    {Py_tp_methods, Multi_methods},
    {Py_tp_getset, Multi_getset},
    {Py_tp_init, Multi_init},
    {Py_tp_new, PyType_GenericNew},
    {Py_tp_dealloc, Multi_dealloc},
    {0, NULL},
};

static PyType_Spec Multi_spec = {"aioquic_amd._crypto.MultiSession", sizeof(MultiObject), 0,
                                 Py_TPFLAGS_DEFAULT, Multi_slots};

/* -------------------------------------------------------- batch calls -- */

/* protect / unprotect(table, desc_ptr, n, in_ptr, out_ptr, res_ptr, stream[, plan]) */
static PyObject *batch_dev(PyObject *args, int enc)
{
    PyObject *t, *po = NULL;
    unsigned long long dp, ip, op, rp, sp;
    unsigned int n;
    if (!PyArg_ParseTuple(args, "OKIKKKK|O", &t, &dp, &n, &ip, &op, &rp, &sp, &po)) return NULL;
    qpp_keytab *kt = as_table(t);
    qpp_plan *plan;
    if (!kt || as_plan(po, &plan) < 0) return NULL;
    int rc = plan ? (enc ? qpp_protect_planned : qpp_unprotect_planned)(
                        kt, plan, as_ptr(dp), n, as_ptr(ip), as_ptr(op), as_ptr(rp), as_ptr(sp))
                  : (enc ? qpp_protect : qpp_unprotect)(kt, as_ptr(dp), n, as_ptr(ip), as_ptr(op),
                                                        as_ptr(rp), as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad batch arguments (n beyond the plan's capacity?)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *py_protect(PyObject *m, PyObject *args) { return batch_dev(args, 1); }
static PyObject *py_unprotect(PyObject *m, PyObject *args) { return batch_dev(args, 0); }

/* plan_build(plan, table, desc_ptr, n, stream) */
static PyObject *py_plan_build(PyObject *m, PyObject *args)
{
    PyObject *po, *t;
    unsigned long long dp, sp;
    unsigned int n;
    if (!PyArg_ParseTuple(args, "OOKIK", &po, &t, &dp, &n, &sp)) return NULL;
    qpp_keytab *kt = as_table(t);
    qpp_plan *plan;
    if (!kt || as_plan(po, &plan) < 0) return NULL;
    if (!plan) {
        PyErr_SetString(PyExc_TypeError, "expected a Plan");
        return NULL;
    }
    int rc = qpp_plan_build(plan, kt, as_ptr(dp), n, as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "batch larger than the plan's capacity");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

/* route(map, cid_len, off_ptr, len_ptr, n, in_ptr, slot_ptr, exp_ptr, n_conn, flags, desc_ptr, route_ptr, stream) */
static PyObject *py_route(PyObject *m, PyObject *args)
{
    PyObject *mo;
    unsigned long long op, lp, ip, slp, ep, dp, rp, sp;
    unsigned int cid_len, n, n_conn, flags;
    if (!PyArg_ParseTuple(args, "OIKKIKKKIIKKK", &mo, &cid_len, &op, &lp, &n, &ip, &slp, &ep, &n_conn, &flags, &dp,
                          &rp, &sp))
        return NULL;
    qpp_cidmap *map = as_cidmap(mo);
    if (!map) return NULL;
    if (flags > 0xffff) {
        PyErr_SetString(PyExc_ValueError, "descriptor flags are 16 bits");
        return NULL;
    }
    int rc = qpp_route(map, cid_len, as_ptr(op), as_ptr(lp), n, as_ptr(ip), as_ptr(slp), as_ptr(ep), n_conn,
                       (uint16_t)flags, as_ptr(dp), as_ptr(rp), as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad route arguments (cid_len outside 1..20, or a null buffer)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}


/* route_unprotect_host(table, map, cid_len, offs_u64, lens_u32, data, conn_slot_u32, conn_expected_u64,
 *                      flags, out_len) -> (out, desc, route, results)
 * route_walk_unprotect_host(table, map, cid_len, offs_u64, lens_u32, data, long_idx_u32, conn_slot_u32 (x KEYSETS),
 *                           conn_expected_u64 (x SPACES), flags, out_len)
 *     -> (out, desc, route, results, walk, walk_n)
 * route_phase_unprotect_host(table, map, cid_len, offs_u64, lens_u32, data, long_idx_u32, conn_slot_u32 (x KEYSETS),
 *                            conn_expected_u64 (x SPACES), conn_next_u32 or None, flags, out_len)
 *     -> (out, desc, route, results, walk, walk_n, phase)
 * One wrapper, as qpp_route.hip's route_unprotect is one session call: the form (0 route, 1 + walk,
 * 2 + walk and phase) says which arrays are parsed, which call runs and how many items come back. */
static PyObject *route_unprotect_host(PyObject *args, int form)
{
    static const char *const refused[3] = {
        "bad route arguments (cid_len outside 1..20, or a datagram outside the input or the output buffer); nothing "
        "was launched",
        "bad route arguments (cid_len outside 1..20, a datagram outside the input or the output buffer, or long_idx "
        "not strictly increasing below n); nothing was launched",
        "bad route arguments (cid_len outside 1..20, a datagram outside the input or the output buffer, long_idx not "
        "strictly increasing below n, or a next-phase slot outside the table); nothing was launched"};
    PyObject *t, *mo;
    const char *offs, *lens, *data, *lidx = NULL, *cslot, *cexp, *cnext = NULL;
    Py_ssize_t l_offs, l_lens, l_data, l_lidx = 0, l_cslot, l_cexp, l_cnext = 0, out_len;
    unsigned int cid_len, flags;
    if (!(form == 0   ? PyArg_ParseTuple(args, "OOIy#y#y#y#y#In", &t, &mo, &cid_len, &offs, &l_offs, &lens, &l_lens,
                                         &data, &l_data, &cslot, &l_cslot, &cexp, &l_cexp, &flags, &out_len)
          : form == 1 ? PyArg_ParseTuple(args, "OOIy#y#y#y#y#y#In", &t, &mo, &cid_len, &offs, &l_offs, &lens, &l_lens,
                                         &data, &l_data, &lidx, &l_lidx, &cslot, &l_cslot, &cexp, &l_cexp, &flags,
                                         &out_len)
                      : PyArg_ParseTuple(args, "OOIy#y#y#y#y#y#z#In", &t, &mo, &cid_len, &offs, &l_offs, &lens,
                                         &l_lens, &data, &l_data, &lidx, &l_lidx, &cslot, &l_cslot, &cexp, &l_cexp,
                                         &cnext, &l_cnext, &flags, &out_len)))
        return NULL;
    qpp_keytab *kt = as_table(t);
    qpp_cidmap *map = kt ? as_cidmap(mo) : NULL;
    if (!map) return NULL;
    /* the walking forms take a slot per key set and an expected number per space of each connection */
    const Py_ssize_t per_slot = form ? 4 * QPP_KEYSETS : 4, per_exp = form ? 8 * QPP_SPACES : 8;
    const Py_ssize_t n = l_lens / 4, nl = l_lidx / 4, nc = l_cslot / per_slot;
    if (l_lens % 4 || l_lidx % 4 || l_cslot != nc * per_slot || l_offs != n * 8 || l_cexp != nc * per_exp ||
        (cnext && l_cnext != nc * 4) || out_len < 0 || flags > 0xffff || n > 0x7fffffff || nc > 0x7fffffff ||
        nl > 0x7fffffff || n + 3 * nl > 0x7fffffff) {
        PyErr_SetString(PyExc_ValueError, "bad array lengths, flags or output length");
        return NULL;
    }
    /* out, desc, route, results, then walk and walk_n, then phase */
    const Py_ssize_t nd = n + 3 * nl, no = form == 0 ? 4 : form == 1 ? 6 : 7;
    const Py_ssize_t size[7] = {out_len,
                                nd * (Py_ssize_t)sizeof(qpp_desc),
                                n * (Py_ssize_t)sizeof(qpp_route_rec),
                                nd * (Py_ssize_t)sizeof(qpp_result),
                                nl * QPP_WALK_MAX * (Py_ssize_t)sizeof(qpp_walk_rec),
                                nl * 4,
                                n};
    PyObject *o[7] = {NULL};
    char *b[7] = {NULL};
    PyObject *ret = PyTuple_New(no);
    for (Py_ssize_t k = 0; ret && k < no; ++k) {
        o[k] = PyBytes_FromStringAndSize(NULL, size[k]);
        if (!o[k] || PyTuple_SetItem(ret, k, o[k]) < 0) Py_CLEAR(ret);
        else b[k] = PyBytes_AsString(o[k]);
    }
    qpp_session *s = ret ? session() : NULL;
    if (!s) {
        Py_XDECREF(ret);
        return NULL;
    }
    /* an empty batch, or a refused one, leaves `out`, `walk` and `phase` as zeros */
    memset(b[0], 0, (size_t)size[0]);
    if (form >= 1) memset(b[4], 0, (size_t)size[4]);
    if (form == 2) memset(b[6], 0, (size_t)size[6]);
    int rc;
    Py_BEGIN_ALLOW_THREADS
    if (form == 0)
        rc = qpp_session_route_unprotect(s, kt, map, cid_len, (const uint64_t *)offs, (const uint32_t *)lens,
                                         (uint32_t)n, (const uint8_t *)data, (size_t)l_data, (const uint32_t *)cslot,
                                         (const uint64_t *)cexp, (uint32_t)nc, (uint16_t)flags, (uint8_t *)b[0],
                                         (size_t)out_len, (qpp_desc *)b[1], (qpp_route_rec *)b[2], (qpp_result *)b[3]);
    else if (form == 1)
        rc = qpp_session_route_walk_unprotect(s, kt, map, cid_len, (const uint64_t *)offs, (const uint32_t *)lens,
                                              (uint32_t)n, (const uint8_t *)data, (size_t)l_data,
                                              (const uint32_t *)lidx, (uint32_t)nl, (const uint32_t *)cslot,
                                              (const uint64_t *)cexp, (uint32_t)nc, (uint16_t)flags, (uint8_t *)b[0],
                                              (size_t)out_len, (qpp_desc *)b[1], (qpp_route_rec *)b[2],
                                              (qpp_result *)b[3], (qpp_walk_rec *)b[4], (uint32_t *)b[5]);
    else
        rc = qpp_session_route_phase_unprotect(s, kt, map, cid_len, (const uint64_t *)offs, (const uint32_t *)lens,
                                               (uint32_t)n, (const uint8_t *)data, (size_t)l_data,
                                               (const uint32_t *)lidx, (uint32_t)nl, (const uint32_t *)cslot,
                                               (const uint64_t *)cexp, (uint32_t)nc, (const uint32_t *)cnext,
                                               (uint16_t)flags, (uint8_t *)b[0], (size_t)out_len, (qpp_desc *)b[1],
                                               (qpp_route_rec *)b[2], (qpp_result *)b[3], (qpp_walk_rec *)b[4],
                                               (uint32_t *)b[5], (uint8_t *)b[6]);
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG) PyErr_SetString(PyExc_ValueError, refused[form]);
    if (rc == QPP_E_ARG || check_rc(rc) < 0) Py_CLEAR(ret);
    return ret;
}

static PyObject *py_route_unprotect_host(PyObject *m, PyObject *args) { return route_unprotect_host(args, 0); }
static PyObject *py_route_walk_unprotect_host(PyObject *m, PyObject *args) { return route_unprotect_host(args, 1); }
static PyObject *py_route_phase_unprotect_host(PyObject *m, PyObject *args) { return route_unprotect_host(args, 2); }

/* route_walk(cid_len, off_ptr, len_ptr, n, in_ptr, route_ptr, long_ptr, n_long, slot_ptr, exp_ptr, n_conn, flags,
 *            desc_ptr, walk_ptr, walk_n_ptr, stream) */
static PyObject *py_route_walk(PyObject *m, PyObject *args)
{
    unsigned long long op, lp, ip, rp, xp, slp, ep, dp, wp, wnp, sp;
    unsigned int cid_len, n, n_long, n_conn, flags;
    if (!PyArg_ParseTuple(args, "IKKIKKKIKKIIKKKK", &cid_len, &op, &lp, &n, &ip, &rp, &xp, &n_long, &slp, &ep, &n_conn,
                          &flags, &dp, &wp, &wnp, &sp))
        return NULL;
    if (flags > 0xffff) {
        PyErr_SetString(PyExc_ValueError, "descriptor flags are 16 bits");
        return NULL;
    }
    int rc = qpp_route_walk(cid_len, as_ptr(op), as_ptr(lp), n, as_ptr(ip), as_ptr(rp), as_ptr(xp), n_long,
                            as_ptr(slp), as_ptr(ep), n_conn, (uint16_t)flags, as_ptr(dp), as_ptr(wp), as_ptr(wnp),
                            as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad route_walk arguments (cid_len outside 1..20, n_long > n, or a null "
                                          "buffer)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}


static PyObject *py_route_walk_launches(PyObject *m, PyObject *unused)
{
    return PyLong_FromUnsignedLongLong(qpp_route_walk_launches());
}

/* route_phase(table, route_ptr (0: one d_next entry per descriptor), next_ptr, n_next, desc_ptr, n, in_ptr,
 *             phase_ptr, stream) */
static PyObject *py_route_phase(PyObject *m, PyObject *args)
{
    PyObject *t;
    unsigned long long rp, np_, dp, ip, pp, sp;
    unsigned int n_next, n;
    if (!PyArg_ParseTuple(args, "OKKIKIKKK", &t, &rp, &np_, &n_next, &dp, &n, &ip, &pp, &sp)) return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    int rc = qpp_route_phase(kt, as_ptr(rp), as_ptr(np_), n_next, as_ptr(dp), n, as_ptr(ip), as_ptr(pp), as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad route_phase arguments (a null buffer)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *py_route_phase_launches(PyObject *m, PyObject *unused)
{
    return PyLong_FromUnsignedLongLong(qpp_route_phase_launches());
}


/* route_accept(off_ptr, len_ptr, n, in_ptr, route_ptr, long_ptr, n_long, walk_ptr, walk_n_ptr, row_ptr, slot_ptr,
 *              n_acc, accept_flags, desc_flags, ini_ptr, desc_ptr, acc_ptr, stream) */
static PyObject *py_route_accept(PyObject *m, PyObject *args)
{
    unsigned long long op, lp, ip, rp, xp, wp, wnp, arp, asp, inip, dp, accp, sp;
    unsigned int n, n_long, n_acc, accept_flags, flags;
    if (!PyArg_ParseTuple(args, "KKIKKKIKKKKIIIKKKK", &op, &lp, &n, &ip, &rp, &xp, &n_long, &wp, &wnp, &arp, &asp,
                          &n_acc, &accept_flags, &flags, &inip, &dp, &accp, &sp))
        return NULL;
    if (flags > 0xffff) {
        PyErr_SetString(PyExc_ValueError, "descriptor flags are 16 bits");
        return NULL;
    }
    int rc = qpp_route_accept(as_ptr(op), as_ptr(lp), n, as_ptr(ip), as_ptr(rp), as_ptr(xp), n_long, as_ptr(wp),
                              as_ptr(wnp), as_ptr(arp), as_ptr(asp), n_acc, accept_flags, (uint16_t)flags,
                              as_ptr(inip), as_ptr(dp), as_ptr(accp), as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad route_accept arguments (a null buffer, or an unknown accept flag)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *py_route_accept_launches(PyObject *m, PyObject *unused)
{
    return PyLong_FromUnsignedLongLong(qpp_route_accept_launches());
}

/* route_reply(off_ptr, len_ptr, n, in_ptr, long_ptr, n_long, walk_ptr, row_ptr, acc_ptr, n_acc, addr_ptr, rand_ptr,
 *             token_ctr, versions_u32, reply_flags, reply_ptr, seal_ptr, tag_ptr, rec_ptr, stream) */
static PyObject *py_route_reply(PyObject *m, PyObject *args)
{
    unsigned long long op, lp, ip, xp, wp, arp, accp, adp, rnp, ctr, rep, sealp, tagp, recp, sp;
    unsigned int n, n_long, n_acc, reply_flags;
    const char *vers;
    Py_ssize_t l_vers;
    if (!PyArg_ParseTuple(args, "KKIKKIKKKIKKKy#IKKKKK", &op, &lp, &n, &ip, &xp, &n_long, &wp, &arp, &accp, &n_acc, &adp,
                          &rnp, &ctr, &vers, &l_vers, &reply_flags, &rep, &sealp, &tagp, &recp, &sp))
        return NULL;
    int rc = l_vers % 4 || l_vers > 4 * QPP_RP_MAX_VERSIONS
                 ? QPP_E_ARG
                 : qpp_route_reply(as_ptr(op), as_ptr(lp), n, as_ptr(ip), as_ptr(xp), n_long, as_ptr(wp), as_ptr(arp),
                                   as_ptr(accp), n_acc, as_ptr(adp), as_ptr(rnp), ctr, (const uint32_t *)vers,
                                   (uint32_t)(l_vers / 4), reply_flags, as_ptr(rep), as_ptr(sealp), as_ptr(tagp),
                                   as_ptr(recp), as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad route_reply arguments (a null buffer, an unknown reply flag, or not "
                                          "1..16 versions)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *py_route_reply_launches(PyObject *m, PyObject *unused)
{
    return PyLong_FromUnsignedLongLong(qpp_route_reply_launches());
}

/* route_token(off_ptr, len_ptr, n, in_ptr, route_ptr, long_ptr, n_long, walk_ptr, walk_n_ptr, row_ptr, n_acc,
 *             accept_flags, tokdesc_ptr, tokrec_ptr, stream) */
static PyObject *py_route_token(PyObject *m, PyObject *args)
{
    unsigned long long op, lp, ip, rp, xp, wp, wnp, arp, tdp, trp, sp;
    unsigned int n, n_long, n_acc, accept_flags;
    if (!PyArg_ParseTuple(args, "KKIKKKIKKKIIKKK", &op, &lp, &n, &ip, &rp, &xp, &n_long, &wp, &wnp, &arp, &n_acc,
                          &accept_flags, &tdp, &trp, &sp))
        return NULL;
    int rc = qpp_route_token(as_ptr(op), as_ptr(lp), n, as_ptr(ip), as_ptr(rp), as_ptr(xp), n_long, as_ptr(wp),
                             as_ptr(wnp), as_ptr(arp), n_acc, accept_flags, as_ptr(tdp), as_ptr(trp), as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad route_token arguments (a null buffer, or an unknown accept flag)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *py_route_token_launches(PyObject *m, PyObject *unused)
{
    return PyLong_FromUnsignedLongLong(qpp_route_token_launches());
}

/* route_accept_tokens(the arguments of route_accept up to desc_flags, addr_ptr, tok_ptr, tokres_ptr, ini_ptr,
 *                     desc_ptr, acc_ptr, tokrec_ptr, stream) */
static PyObject *py_route_accept_tokens(PyObject *m, PyObject *args)
{
    unsigned long long op, lp, ip, rp, xp, wp, wnp, arp, asp, adp, tkp, trsp, inip, dp, accp, trp, sp;
    unsigned int n, n_long, n_acc, accept_flags, flags;
    if (!PyArg_ParseTuple(args, "KKIKKKIKKKKIIIKKKKKKKK", &op, &lp, &n, &ip, &rp, &xp, &n_long, &wp, &wnp, &arp, &asp,
                          &n_acc, &accept_flags, &flags, &adp, &tkp, &trsp, &inip, &dp, &accp, &trp, &sp))
        return NULL;
    if (flags > 0xffff) {
        PyErr_SetString(PyExc_ValueError, "descriptor flags are 16 bits");
        return NULL;
    }
    int rc = qpp_route_accept_tokens(as_ptr(op), as_ptr(lp), n, as_ptr(ip), as_ptr(rp), as_ptr(xp), n_long,
                                     as_ptr(wp), as_ptr(wnp), as_ptr(arp), as_ptr(asp), n_acc, accept_flags,
                                     (uint16_t)flags, as_ptr(adp), as_ptr(tkp), as_ptr(trsp), as_ptr(inip), as_ptr(dp),
                                     as_ptr(accp), as_ptr(trp), as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError,
                        "bad route_accept_tokens arguments (a null buffer, or an unknown accept flag)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static int host_call(int enc, qpp_keytab *kt, const void *desc, uint32_t n, const void *in,
                     size_t in_len, void *out, size_t out_len, void *res)
{
    qpp_session *s = session();
    if (!s) return -1;
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = enc ? qpp_session_protect(s, kt, desc, n, in, in_len, out, out_len, res)
             : qpp_session_unprotect(s, kt, desc, n, in, in_len, out, out_len, res);
    Py_END_ALLOW_THREADS
    return check_rc(rc);
}

/* protect_host / unprotect_host(table, desc, data, out_len) -> (out, results) */
static PyObject *batch_host(PyObject *args, int enc)
{
    PyObject *t;
    const char *desc, *data;
    Py_ssize_t desc_len, data_len, out_len;
    if (!PyArg_ParseTuple(args, "Oy#y#n", &t, &desc, &desc_len, &data, &data_len, &out_len))
        return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    if (desc_len % (Py_ssize_t)sizeof(qpp_desc) || out_len < 0) {
        PyErr_SetString(PyExc_ValueError, "bad descriptor buffer or output length");
        return NULL;
    }
    uint32_t n = (uint32_t)(desc_len / (Py_ssize_t)sizeof(qpp_desc));
    PyObject *out = PyBytes_FromStringAndSize(NULL, out_len);
    PyObject *res = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)n * (Py_ssize_t)sizeof(qpp_result));
    PyObject *ret = NULL;
    if (out && res) {
        char *o = PyBytes_AsString(out);
        /* the session writes every byte of out (zeros where no packet lands)
           for n > 0, so only an empty batch needs the zero fill here */
        if (n == 0) memset(o, 0, (size_t)out_len);
        if (host_call(enc, kt, desc, n, data, (size_t)data_len, o, (size_t)out_len,
                      PyBytes_AsString(res)) == 0)
            ret = PyTuple_Pack(2, out, res);
    }
    Py_XDECREF(out);
    Py_XDECREF(res);
    return ret;
}

static PyObject *py_protect_host(PyObject *m, PyObject *args) { return batch_host(args, 1); }
static PyObject *py_unprotect_host(PyObject *m, PyObject *args) { return batch_host(args, 0); }

/* protect_into / unprotect_into(table, desc_ptr, n, in_ptr, in_len, out_ptr,
   out_len, res_ptr): host memory given by address (e.g. numpy arrays reused
   across batches), so a large batch neither allocates nor first-touches a
   fresh bytes object per call.  The caller keeps the memory alive. */
static PyObject *batch_into(PyObject *args, int enc)
{
    PyObject *t;
    unsigned long long dp, ip, op, rp, in_len, out_len;
    unsigned int n;
    if (!PyArg_ParseTuple(args, "OKIKKKKK", &t, &dp, &n, &ip, &in_len, &op, &out_len, &rp))
        return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    if (n == 0) {
        if (out_len) memset(as_ptr(op), 0, (size_t)out_len);
        Py_RETURN_NONE;
    }
    if (!dp || !rp || (in_len && !ip) || (out_len && !op)) {
        PyErr_SetString(PyExc_ValueError, "null buffer");
        return NULL;
    }
    if (host_call(enc, kt, as_ptr(dp), n, as_ptr(ip), (size_t)in_len, as_ptr(op), (size_t)out_len,
                  as_ptr(rp)) < 0)
        return NULL;
    Py_RETURN_NONE;
}

static PyObject *py_protect_into(PyObject *m, PyObject *args) { return batch_into(args, 1); }
static PyObject *py_unprotect_into(PyObject *m, PyObject *args) { return batch_into(args, 0); }

/* protect_list(table, slots_u32, pns_u64, headers, payloads) -> (wires, results)
 * unprotect_list(table, slots_u32, expected_u64, packets, pn_offs_u32)
 *     -> (list of (plain_header, payload) or None, results)
 * The batched callers' form: the packets are copied straight from the bytes
 * objects of the lists into the session's pinned staging buffer, and the
 * outputs are cut straight from its pinned output buffer, one bytes object
 * each; no intermediate joins or slices in Python. */
static PyObject *batch_list(PyObject *args, int enc)
{
    PyObject *t, *items;
    const char *slots, *nums, *extra = NULL;
    Py_ssize_t slots_len, nums_len, extra_len = 0;
    PyObject *payloads = NULL;
    if (enc) {
        if (!PyArg_ParseTuple(args, "Oy#y#O!O!", &t, &slots, &slots_len, &nums, &nums_len, &PyList_Type,
                              &items, &PyList_Type, &payloads))
            return NULL;
    } else if (!PyArg_ParseTuple(args, "Oy#y#O!y#", &t, &slots, &slots_len, &nums, &nums_len, &PyList_Type,
                                 &items, &extra, &extra_len)) {
        return NULL;
    }
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    const Py_ssize_t n = PyList_Size(items);
    if (slots_len != 4 * n || nums_len != 8 * n || (enc ? PyList_Size(payloads) != n : extra_len != 4 * n)) {
        PyErr_SetString(PyExc_ValueError, "per-packet arrays do not match the packet list");
        return NULL;
    }
    if (n > 0x7fffffff) {
        PyErr_SetString(PyExc_ValueError, "batch too large");
        return NULL;
    }
    /* first pass: sizes (and the type check of every item) */
    size_t total = 0;
    for (Py_ssize_t i = 0; i < n; ++i) {
        char *b;
        Py_ssize_t l1, l2 = 0;
        if (PyBytes_AsStringAndSize(PyList_GetItem(items, i), &b, &l1) < 0) return NULL;
        if (enc && PyBytes_AsStringAndSize(PyList_GetItem(payloads, i), &b, &l2) < 0) return NULL;
        /* protect: up to 15 bytes of room to start each payload on a
           16-byte boundary (Payload alignment) */
        total += (size_t)l1 + (size_t)l2 + (enc ? QPP_TAG_LEN + 15 : 0);
    }
    qpp_session *s = session();
    if (!s) return NULL;
    PyObject *res = PyBytes_FromStringAndSize(NULL, n * (Py_ssize_t)sizeof(qpp_result));
    qpp_desc *desc = (qpp_desc *)calloc(n ? (size_t)n : 1, sizeof(qpp_desc));
    uint8_t *hin = NULL, *hout = NULL;
    PyObject *ret = NULL, *outs = NULL;
    if (!res || !desc) {
        PyErr_NoMemory();
        goto done;
    }
    if (n == 0) {
        outs = PyList_New(0);
        goto pack;
    }
    if (check_rc(qpp_session_stage(s, total ? total : 1, (uint32_t)n, &hin, &hout)) < 0) goto done;
    {
        const uint32_t *sl = (const uint32_t *)slots;
        size_t off = 0;
        for (Py_ssize_t i = 0; i < n; ++i) {
            char *b1, *b2 = NULL;
            Py_ssize_t l1, l2 = 0;
            (void)PyBytes_AsStringAndSize(PyList_GetItem(items, i), &b1, &l1);
            if (enc) (void)PyBytes_AsStringAndSize(PyList_GetItem(payloads, i), &b2, &l2);
            qpp_desc *d = &desc[i];
            if (enc) off = ((off + (size_t)l1 + 15) & ~(size_t)15) - (size_t)l1;
            d->in_off = d->out_off = off;
            uint64_t num;
            memcpy(&num, nums + 8 * i, 8);
            d->pn = num;
            d->slot = sl[i];
            memcpy(hin + off, b1, (size_t)l1);
            if (enc) {
                /* a header the 16-bit field cannot carry is rejected below */
                d->hdr_len = l1 > 0xffff ? 0xffff : (uint16_t)l1;
                d->len = (uint32_t)l2;
                memcpy(hin + off + l1, b2, (size_t)l2);
                off += (size_t)l1 + (size_t)l2 + QPP_TAG_LEN;
            } else {
                uint32_t po;
                memcpy(&po, extra + 4 * i, 4);
                d->hdr_len = po > 0xffff ? 0xffff : (uint16_t)po;
                d->len = (uint32_t)l1;
                off += (size_t)l1;
            }
        }
    }
    if (host_call(enc, kt, desc, (uint32_t)n, hin, total, hout, total, PyBytes_AsString(res)) < 0) goto done;
    outs = PyList_New(n);
    if (!outs) goto done;
    {
        const qpp_result *r = (const qpp_result *)PyBytes_AsString(res);
        for (Py_ssize_t i = 0; i < n; ++i) {
            const uint8_t *o = hout + desc[i].out_off;
            PyObject *item;
            if (enc) {
                item = PyBytes_FromStringAndSize((const char *)o, (Py_ssize_t)desc[i].hdr_len + desc[i].len +
                                                                      QPP_TAG_LEN);
            } else if (r[i].status == QPP_S_OK) {
                PyObject *h = PyBytes_FromStringAndSize((const char *)o, r[i].hdr_len);
                PyObject *p = PyBytes_FromStringAndSize((const char *)o + r[i].hdr_len,
                                                        (Py_ssize_t)r[i].out_len - r[i].hdr_len);
                item = (h && p) ? PyTuple_Pack(2, h, p) : NULL;
                Py_XDECREF(h);
                Py_XDECREF(p);
                if (item) PyObject_GC_UnTrack(item); /* two bytes objects: never in a cycle */
            } else {
                Py_INCREF(Py_None);
                item = Py_None;
            }
            if (!item) {
                Py_CLEAR(outs);
                goto done;
            }
            PyList_SetItem(outs, i, item); /* steals */
        }
    }
pack:
    if (outs) ret = PyTuple_Pack(2, outs, res);
done:
    Py_XDECREF(outs);
    Py_XDECREF(res);
    free(desc);
    return ret;
}

static PyObject *py_protect_list(PyObject *m, PyObject *args) { return batch_list(args, 1); }
static PyObject *py_unprotect_list(PyObject *m, PyObject *args) { return batch_list(args, 0); }

/* A per-packet array argument ("y#": any read-only bytes-like object)
 * must hold exactly n items of `size` bytes. */
static int check_len(Py_ssize_t len, Py_ssize_t n, Py_ssize_t size, const char *what)
{
    if (len == n * size) return 0;
    PyErr_Format(PyExc_ValueError, "%s: %zd bytes for %zd items of %zd", what, len, n, size);
    return -1;
}

/* The scratch of one call: every buffer it takes, released together.  A failed
 * allocation is remembered, so a caller takes all it needs and asks once. */
#define SCRATCH_MAX 32
typedef struct {
    void *p[SCRATCH_MAX];
    int n, failed;
} Scratch;

static void *scratch_alloc(Scratch *s, size_t bytes, int zeroed)
{
    void *p = NULL;
    if (s->n < SCRATCH_MAX) p = zeroed ? calloc(bytes ? bytes : 1, 1) : malloc(bytes ? bytes : 1);
    if (p) s->p[s->n++] = p;
    else s->failed = 1;
    return p;
}

#define SCRATCH(s, type, count) ((type *)scratch_alloc((s), (size_t)(count) * sizeof(type), 0))
#define SCRATCH0(s, type, count) ((type *)scratch_alloc((s), (size_t)(count) * sizeof(type), 1))

static void scratch_free_all(Scratch *s)
{
    while (s->n) free(s->p[--s->n]);
}

/* protect_datagrams(table, plains, dg_u32, off_u32, hsize_u32, size_u32, pn_u64, slot_u32)
 *     -> (wire datagrams, results)
 * The deferred-encryption builder's flush (QuicPacketBuilder._end_packet,
 * packet_builder.py:341-350, for every packet of every datagram at once):
 * the plaintext datagrams go back to back into the session's pinned staging;
 * packet k of datagram dg[k] starts at off[k] with hsize[k] header bytes and
 * size[k] header + payload bytes (its tag's room follows).  Each wire
 * datagram comes back as one bytes object cut from the pinned output, which
 * the session writes in full (zeros outside packets: the builder's datagram
 * padding is zeros too). */
static PyObject *py_protect_datagrams(PyObject *m, PyObject *args)
{
    PyObject *t, *plains;
    const char *a_dg, *a_off, *a_hs, *a_sz, *a_pn, *a_sl;
    Py_ssize_t l_dg, l_off, l_hs, l_sz, l_pn, l_sl;
    if (!PyArg_ParseTuple(args, "OO!y#y#y#y#y#y#", &t, &PyList_Type, &plains, &a_dg, &l_dg, &a_off, &l_off, &a_hs,
                          &l_hs, &a_sz, &l_sz, &a_pn, &l_pn, &a_sl, &l_sl))
        return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    const Py_ssize_t n = l_dg / 4;
    if (check_len(l_dg, n, 4, "dg") < 0 || check_len(l_off, n, 4, "off") < 0 || check_len(l_hs, n, 4, "hsize") < 0 ||
        check_len(l_sz, n, 4, "size") < 0 || check_len(l_pn, n, 8, "pn") < 0 || check_len(l_sl, n, 4, "slot") < 0)
        return NULL;
    /* a snapshot holding a reference to every datagram: the copies below run
       without the GIL, while another thread may change the caller's list */
    plains = PySequence_Tuple(plains);
    if (!plains) return NULL;
    const Py_ssize_t nd = PyTuple_Size(plains);
    PyObject *ret = NULL, *wires = NULL;
    Scratch sc = {{NULL}, 0, 0};
    size_t *base = SCRATCH(&sc, size_t, nd + 1);
    qpp_desc *desc = SCRATCH0(&sc, qpp_desc, n);
    /* the copy jobs: datagram d between its bytes object and staging */
    uint8_t **cd = SCRATCH(&sc, uint8_t *, nd + 1);
    const uint8_t **cs = SCRATCH(&sc, const uint8_t *, nd + 1);
    size_t *cl = SCRATCH(&sc, size_t, nd + 1);
    PyObject *res = PyBytes_FromStringAndSize(NULL, n * (Py_ssize_t)sizeof(qpp_result));
    if (sc.failed || !res) {
        PyErr_NoMemory();
        goto done;
    }
    base[0] = 0;
    for (Py_ssize_t d = 0; d < nd; ++d) {
        PyObject *o = PyTuple_GetItem(plains, d);
        if (!PyBytes_Check(o)) {
            PyErr_SetString(PyExc_TypeError, "datagrams must be bytes");
            goto done;
        }
        base[d + 1] = base[d] + (size_t)PyBytes_Size(o);
    }
    {
        const uint32_t *dg = (const uint32_t *)a_dg, *off = (const uint32_t *)a_off, *hs = (const uint32_t *)a_hs,
                       *sz = (const uint32_t *)a_sz, *sl = (const uint32_t *)a_sl;
        const uint64_t *pn = (const uint64_t *)a_pn;
        for (Py_ssize_t k = 0; k < n; ++k) {
            if (dg[k] >= (uint32_t)nd || hs[k] > sz[k] ||
                (size_t)off[k] + sz[k] + QPP_TAG_LEN > base[dg[k] + 1] - base[dg[k]]) {
                PyErr_SetString(PyExc_ValueError, "packet outside its datagram");
                goto done;
            }
            qpp_desc *x = &desc[k];
            x->in_off = x->out_off = base[dg[k]] + off[k];
            x->hdr_len = hs[k] > 0xffff ? 0xffff : (uint16_t)hs[k];
            x->len = sz[k] - hs[k];
            x->pn = pn[k];
            x->slot = sl[k];
        }
    }
    {
        const size_t total = base[nd];
        qpp_session *s = session();
        uint8_t *hin, *hout;
        if (!s || check_rc(qpp_session_stage(s, total ? total : 1, (uint32_t)(n ? n : 1), &hin, &hout)) < 0)
            goto done;
        for (Py_ssize_t d = 0; d < nd; ++d) {
            cd[d] = hin + base[d];
            cs[d] = (const uint8_t *)PyBytes_AsString(PyTuple_GetItem(plains, d));
            cl[d] = base[d + 1] - base[d];
        }
        Py_BEGIN_ALLOW_THREADS  /* the snapshot holds every datagram */
        par_copy(cd, cs, cl, (size_t)nd, total);
        Py_END_ALLOW_THREADS
        const uint8_t *src = hin;  /* no packet: the datagrams as they are */
        int ok = 1;
        if (n) {
            ok = host_call(1, kt, desc, (uint32_t)n, hin, total, hout, total, PyBytes_AsString(res)) == 0;
            src = hout;
        }
        if (ok) wires = PyList_New(nd);
        for (Py_ssize_t d = 0; wires && d < nd; ++d) {
            /* allocated here, filled below without the GIL (not yet shared) */
            PyObject *o = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)cl[d]);
            if (!o) {
                Py_CLEAR(wires);
                break;
            }
            PyList_SetItem(wires, d, o);
            cd[d] = (uint8_t *)PyBytes_AsString(o);
            cs[d] = src + base[d];
        }
        if (wires) {
            Py_BEGIN_ALLOW_THREADS
            par_copy(cd, cs, cl, (size_t)nd, total);
            Py_END_ALLOW_THREADS
            ret = PyTuple_Pack(2, wires, res);
        }
    }
done:
    Py_XDECREF(wires);
    Py_XDECREF(res);
    Py_DECREF(plains);
    scratch_free_all(&sc);
    return ret;
}

/* ---- routed send: headers and packet numbers built on the device ---- */

/* send_fill(table, sendconn_ptr, n_conn, off_ptr, len_ptr, conn_ptr, seq_ptr, n, buf_ptr, buf_len, desc_ptr,
 *           rec_ptr, stream) */
static PyObject *py_send_fill(PyObject *m, PyObject *args)
{
    PyObject *t;
    unsigned long long cp, op, lp, ip, qp, bp, buf_len, dp, rp, sp;
    unsigned int n_conn, n;
    if (!PyArg_ParseTuple(args, "OKIKKKKIKKKKK", &t, &cp, &n_conn, &op, &lp, &ip, &qp, &n, &bp, &buf_len, &dp, &rp,
                          &sp))
        return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    int rc = qpp_send_fill(kt, as_ptr(cp), n_conn, as_ptr(op), as_ptr(lp), as_ptr(ip), as_ptr(qp), n, as_ptr(bp),
                           buf_len, as_ptr(dp), as_ptr(rp), as_ptr(sp));
    if (rc == QPP_E_ARG) {
        PyErr_SetString(PyExc_ValueError, "bad send_fill arguments (a null buffer)");
        return NULL;
    }
    if (check_rc(rc) < 0) return NULL;
    Py_RETURN_NONE;
}

static PyObject *py_send_launches(PyObject *m, PyObject *unused)
{
    return PyLong_FromUnsignedLongLong(qpp_send_launches());
}

static const char *const k_send_refused =
    "bad send arguments (offsets not strictly increasing, a packet's region overlapping its predecessor's or outside "
    "the input or the output buffer, a connection index out of range, or a slot outside the table); nothing was "
    "launched";

/* send_protect_host(table, sendconn, off_u64, len_u32, conn_u32, seq_u32, data, out_len)
 *     -> (out, desc, records, results)
 * qpp_session_send_protect over the caller's own arrays and staged buffer. */
static PyObject *py_send_protect_host(PyObject *m, PyObject *args)
{
    PyObject *t;
    const char *sc, *offs, *lens, *conns, *seqs, *data;
    Py_ssize_t l_sc, l_offs, l_lens, l_conns, l_seqs, l_data, out_len;
    if (!PyArg_ParseTuple(args, "Oy#y#y#y#y#y#n", &t, &sc, &l_sc, &offs, &l_offs, &lens, &l_lens, &conns, &l_conns,
                          &seqs, &l_seqs, &data, &l_data, &out_len))
        return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    const Py_ssize_t n = l_lens / 4, nc = l_sc / (Py_ssize_t)sizeof(qpp_send_conn);
    if (check_len(l_sc, nc, sizeof(qpp_send_conn), "sendconn") < 0 || check_len(l_offs, n, 8, "off") < 0 ||
        check_len(l_lens, n, 4, "len") < 0 || check_len(l_conns, n, 4, "conn") < 0 ||
        check_len(l_seqs, n, 4, "seq") < 0)
        return NULL;
    if (out_len < 0 || n > 0x7fffffff || nc > 0x7fffffff) {
        PyErr_SetString(PyExc_ValueError, "bad array lengths or output length");
        return NULL;
    }
    const Py_ssize_t size[4] = {out_len, n * (Py_ssize_t)sizeof(qpp_desc), n * (Py_ssize_t)sizeof(qpp_send_rec),
                                n * (Py_ssize_t)sizeof(qpp_result)};
    char *b[4] = {NULL};
    PyObject *ret = PyTuple_New(4);
    for (Py_ssize_t k = 0; ret && k < 4; ++k) {
        PyObject *o = PyBytes_FromStringAndSize(NULL, size[k]);
        if (!o || PyTuple_SetItem(ret, k, o) < 0) Py_CLEAR(ret);
        else b[k] = PyBytes_AsString(o);
    }
    qpp_session *s = ret ? session() : NULL;
    if (!s) {
        Py_XDECREF(ret);
        return NULL;
    }
    memset(b[0], 0, (size_t)size[0]);  /* an empty batch leaves `out` as zeros */
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = qpp_session_send_protect(s, kt, (const qpp_send_conn *)sc, (uint32_t)nc, (const uint64_t *)offs,
                                  (const uint32_t *)lens, (const uint32_t *)conns, (const uint32_t *)seqs, (uint32_t)n,
                                  (const uint8_t *)data, (size_t)l_data, (uint8_t *)b[0], (size_t)out_len,
                                  (qpp_desc *)b[1], (qpp_send_rec *)b[2], (qpp_result *)b[3]);
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG) PyErr_SetString(PyExc_ValueError, k_send_refused);
    if (rc == QPP_E_ARG || check_rc(rc) < 0) Py_CLEAR(ret);
    return ret;
}

/* send_routed(table, sendconn, conn_u32, payloads) -> (datagrams, records, results)
 * The batched sender without a host header pass: payload k (bytes) of
 * connection conn[k] is staged into the session's pinned input at an offset
 * computed here, QPP_SEND_HEAD bytes before it and QPP_SEND_TAIL after it
 * free; its ordinal among its connection's payloads is counted in the same
 * pass; qpp_session_send_protect builds the headers, numbers and padding and
 * seals the packets.  Each datagram comes back as one bytes object cut from
 * the pinned output (b"" for a packet whose record or result is not OK). */
static PyObject *py_send_routed(PyObject *m, PyObject *args)
{
    PyObject *t, *payloads;
    const char *a_sc, *a_conn;
    Py_ssize_t l_sc, l_conn;
    if (!PyArg_ParseTuple(args, "Oy#y#O!", &t, &a_sc, &l_sc, &a_conn, &l_conn, &PyList_Type, &payloads)) return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    const Py_ssize_t n = l_conn / 4, nc = l_sc / (Py_ssize_t)sizeof(qpp_send_conn);
    if (check_len(l_sc, nc, sizeof(qpp_send_conn), "sendconn") < 0 || check_len(l_conn, n, 4, "conn") < 0) return NULL;
    /* a snapshot holding a reference to every payload: the copies below run
       without the GIL, while another thread may change the caller's list */
    payloads = PySequence_Tuple(payloads);
    if (!payloads) return NULL;
    PyObject *ret = NULL, *wires = NULL, *rec = NULL, *res = NULL;
    Scratch sc = {{NULL}, 0, 0};
    if (PyTuple_Size(payloads) != n || n > 0x7fffffff || nc > 0x7fffffff) {
        PyErr_SetString(PyExc_ValueError, "one connection index per payload");
        goto done;
    }
    uint64_t *off = SCRATCH(&sc, uint64_t, n + 1);
    uint32_t *len = SCRATCH(&sc, uint32_t, n + 1);
    uint32_t *seq = SCRATCH(&sc, uint32_t, n + 1);
    uint32_t *count = SCRATCH0(&sc, uint32_t, nc + 1);
    uint8_t **cd = SCRATCH(&sc, uint8_t *, n + 1);
    const uint8_t **cs = SCRATCH(&sc, const uint8_t *, n + 1);
    size_t *cl = SCRATCH(&sc, size_t, n + 1);
    rec = PyBytes_FromStringAndSize(NULL, n * (Py_ssize_t)sizeof(qpp_send_rec));
    res = PyBytes_FromStringAndSize(NULL, n * (Py_ssize_t)sizeof(qpp_result));
    if (sc.failed || !rec || !res) {
        PyErr_NoMemory();
        goto done;
    }
    const uint32_t *conn = (const uint32_t *)a_conn;
    size_t total = 0, bytes = 0;
    for (Py_ssize_t k = 0; k < n; ++k) {
        PyObject *o = PyTuple_GetItem(payloads, k);
        if (!PyBytes_Check(o) || PyBytes_Size(o) > QPP_PACKET_MAX) {
            PyErr_SetString(PyExc_TypeError, "payloads must be bytes of at most 1500");
            goto done;
        }
        len[k] = (uint32_t)PyBytes_Size(o);
        off[k] = total + QPP_SEND_HEAD;
        total = (size_t)off[k] + len[k] + QPP_SEND_TAIL;
        bytes += len[k];
        /* (an index out of range is refused by the session's check below) */
        seq[k] = conn[k] < (uint32_t)nc ? count[conn[k]]++ : 0;
    }
    {
        qpp_session *s = session();
        uint8_t *hin, *hout;
        if (!s || check_rc(qpp_session_stage(s, total ? total : 1, (uint32_t)(n ? n : 1), &hin, &hout)) < 0) goto done;
        for (Py_ssize_t k = 0; k < n; ++k) {
            cd[k] = hin + off[k];
            cs[k] = (const uint8_t *)PyBytes_AsString(PyTuple_GetItem(payloads, k));
            cl[k] = len[k];
        }
        qpp_send_rec *rr = (qpp_send_rec *)PyBytes_AsString(rec);
        qpp_result *rs = (qpp_result *)PyBytes_AsString(res);
        int rc;
        Py_BEGIN_ALLOW_THREADS  /* the snapshot holds every payload */
        par_copy(cd, cs, cl, (size_t)n, bytes);
        rc = qpp_session_send_protect(s, kt, (const qpp_send_conn *)a_sc, (uint32_t)nc, off, len, conn, seq,
                                      (uint32_t)n, hin, total, hout, total, NULL, rr, rs);
        Py_END_ALLOW_THREADS
        if (rc == QPP_E_ARG) PyErr_SetString(PyExc_ValueError, k_send_refused);
        if (rc == QPP_E_ARG || check_rc(rc) < 0) goto done;
        wires = PyList_New(n);
        bytes = 0;
        for (Py_ssize_t k = 0; wires && k < n; ++k) {
            const int ok = rr[k].status == QPP_SN_OK && rs[k].status == QPP_S_OK;
            cl[k] = ok ? rs[k].out_len : 0;
            /* allocated here, filled below without the GIL (not yet shared) */
            PyObject *o = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)cl[k]);
            if (!o) {
                Py_CLEAR(wires);
                break;
            }
            PyList_SetItem(wires, k, o);
            cd[k] = (uint8_t *)PyBytes_AsString(o);
            cs[k] = hout + off[k] - rr[k].hdr_len;
            bytes += cl[k];
        }
        if (wires) {
            Py_BEGIN_ALLOW_THREADS
            par_copy(cd, cs, cl, (size_t)n, bytes);
            Py_END_ALLOW_THREADS
            ret = PyTuple_Pack(3, wires, rec, res);
        }
    }
done:
    Py_XDECREF(wires);
    Py_XDECREF(rec);
    Py_XDECREF(res);
    Py_DECREF(payloads);
    scratch_free_all(&sc);
    return ret;
}

/* receive_short's slot_of: closed on entry / no receive key (no launch) */
#define RS_CLOSED 0xfffffffeu

/* What a walk starts from and hands back: copies of the caller's expected
 * numbers and closed flags for qpp_rxwalk.h's rule to update, nothing blocked. */
typedef struct {
    RxWalkState st;
    PyObject *sexp, *closed;
} WalkState;

static int walk_state_init(WalkState *ws, Scratch *sc, const char *a_sexp, Py_ssize_t l_sexp, const char *a_closed,
                           Py_ssize_t l_closed, size_t n_pairs)
{
    ws->sexp = PyBytes_FromStringAndSize(a_sexp, l_sexp);
    ws->closed = PyBytes_FromStringAndSize(a_closed, l_closed);
    if (!ws->sexp || !ws->closed) return -1;
    ws->st.sx = (uint64_t *)PyBytes_AsString(ws->sexp);
    ws->st.closed = (uint8_t *)PyBytes_AsString(ws->closed);
    ws->st.blocked_pair = SCRATCH0(sc, uint8_t, n_pairs);
    ws->st.blocked_space = SCRATCH0(sc, uint8_t, l_sexp / 8);
    ws->st.blocked_conn = SCRATCH0(sc, uint8_t, l_closed);
    ws->st.rolled = NULL;
    return sc->failed ? (PyErr_NoMemory(), -1) : 0;
}

static void walk_state_clear(WalkState *ws)
{
    Py_CLEAR(ws->sexp);
    Py_CLEAR(ws->closed);
}

/* The in-order walk of unprotect_walk / walk_results over the results of one
 * launch: r[i] (statuses rewritten in place) and the output of packet i at
 * hout + out_off[i]. */
typedef struct {
    Py_ssize_t n;
    const uint32_t *slots, *offs, *pair, *space, *conn;
    const uint64_t *exp, *out_off;
    const uint8_t *track, *rsv, *hout;
    RxWalkState *st;
    PyObject *outs, *deferred;
} ResultsWalk;

static int results_walk(const ResultsWalk *w, qpp_result *r)
{
    /* no receive key (crypto.py:78-79) and packet-number offsets past the
       header limit fail whatever the launch left in their results */
    for (Py_ssize_t i = 0; i < w->n; ++i) {
        if (w->slots[i] == 0xffffffffu) r[i].status = QPP_S_NO_KEY;
        else if (w->offs[i] > QPP_MAX_HDR) r[i].status = QPP_S_LENGTH;
    }
    for (Py_ssize_t i = 0; i < w->n; ++i) {
        RxWalkPacket f = {.pair = w->pair[i], .space = w->space[i], .conn = w->conn[i], .launched = 1,
                          .status = r[i].status, .hdr_len = r[i].hdr_len, .pn = r[i].pn, .pn_off = w->offs[i],
                          .exp = w->exp[i], .rsv_mask = w->rsv[i], .track = w->track[i], .phase = RXWALK_NO_PHASE};
        const uint8_t *o = f.status == QPP_S_OK ? w->hout + w->out_off[i] : NULL;
        if (o && f.hdr_len) f.first = o[0];
        Py_INCREF(Py_None);
        PyList_SetItem(w->outs, i, Py_None);
        switch (rxwalk_step(w->st, &f)) {
        case RXW_DEFERRED: {
            PyObject *ix = PyLong_FromSsize_t(i);
            const int bad = ix ? PyList_Append(w->deferred, ix) : -1;
            Py_XDECREF(ix);
            if (bad < 0) return -1;
            break;
        }
        case RXW_CLOSED: r[i].status = WALK_S_CLOSED; break;
        case RXW_RESERVED: r[i].status = WALK_S_RESERVED; break;
        case RXW_OK: {
            PyObject *h = PyBytes_FromStringAndSize((const char *)o, f.hdr_len);
            PyObject *pl = PyBytes_FromStringAndSize((const char *)o + f.hdr_len, (Py_ssize_t)r[i].out_len - f.hdr_len);
            PyObject *pn = PyLong_FromUnsignedLongLong(f.pn);
            PyObject *item = (h && pl && pn) ? PyTuple_Pack(3, h, pl, pn) : NULL;
            Py_XDECREF(h);
            Py_XDECREF(pl);
            Py_XDECREF(pn);
            if (!item) return -1;
            PyObject_GC_UnTrack(item); /* bytes and an int: never in a cycle (make_record) */
            PyList_SetItem(w->outs, i, item);
            break;
        }
        default: break; /* no key, or failed: the status says which */
        }
    }
    return 0;
}

/* The per-packet arrays of unprotect_walk and walk_results hold n items each. */
static int walk_lens_ok(Py_ssize_t n, Py_ssize_t l_sl, Py_ssize_t l_exp, Py_ssize_t l_offs, Py_ssize_t l_pair,
                        Py_ssize_t l_space, Py_ssize_t l_track, Py_ssize_t l_conn, Py_ssize_t l_rsv, Py_ssize_t l_sexp)
{
    if (l_sexp % 8) {
        PyErr_SetString(PyExc_ValueError, "space_exp: whole u64 items");
        return 0;
    }
    return check_len(l_sl, n, 4, "slots") == 0 && check_len(l_exp, n, 8, "exp") == 0 &&
           check_len(l_offs, n, 4, "offs") == 0 && check_len(l_pair, n, 4, "pair") == 0 &&
           check_len(l_space, n, 4, "space") == 0 && check_len(l_track, n, 1, "track") == 0 &&
           check_len(l_conn, n, 4, "conn") == 0 && check_len(l_rsv, n, 1, "rsv") == 0;
}


/* unprotect_walk(table, slots_u32, exp_u64, packets, offs_u32, pair_u32,
 *                space_u32, track_u8, space_exp_u64, n_pairs, conn_u32,
 *                rsv_u8, closed_u8)
 *     -> (outcomes, results, deferred, space_exp_u64 after the walk,
 *         closed_u8 after the walk)
 * One ReceiveBatch round in C: the launch (as unprotect_list, each packet
 * decoded against exp[i], its space's expected number when the round began)
 * and the in-order walk of CryptoPair.decrypt_packet semantics
 * (quic/crypto.py:184-192, connection.py:905-947,984-985) for every packet
 * whose outcome does not depend on a state change this round makes:
 *   outcomes[i] = (plain_header, payload, packet_number) on success, None on
 *   failure (results[i].status says which), or None for a deferred packet;
 *   the returned copy of space_exp advances as connection.py:984-985 does
 *   (for track[i]).
 * A packet is deferred -- and with it every later packet of its pair and of
 * its space -- when its key phase flipped (a key roll follows), or when its
 * truncated number decodes differently under the space's expected number by
 * now than under exp[i].  The caller's general walk (batch_io.ReceiveBatch)
 * then continues with the deferred packets, in order, from the state left
 * here.
 * Connections (conn_u32[i]: the packet's connection, WALK_NO_CONN for none;
 * rsv_u8[i]: its reserved-bit mask, 0 for no check; closed_u8: each
 * connection's closed flag, returned updated): a packet that authenticates
 * with a reserved bit set closes its connection (connection.py:949-960) --
 * status WALK_S_RESERVED, no expected-number update -- and every later packet
 * of a closed connection gets WALK_S_CLOSED (:756-757).  A deferred packet
 * blocks its connection too: whether it closes it is not known yet. */
static PyObject *py_unprotect_walk(PyObject *m, PyObject *args)
{
    PyObject *t, *packets;
    const char *a_sl, *a_exp, *a_offs, *a_pair, *a_space, *a_track, *a_sexp, *a_conn, *a_rsv, *a_closed;
    Py_ssize_t l_sl, l_exp, l_offs, l_pair, l_space, l_track, l_sexp, l_conn, l_rsv, l_closed;
    unsigned int n_pairs;
    if (!PyArg_ParseTuple(args, "Oy#y#O!y#y#y#y#y#Iy#y#y#", &t, &a_sl, &l_sl, &a_exp, &l_exp, &PyList_Type, &packets,
                          &a_offs, &l_offs, &a_pair, &l_pair, &a_space, &l_space, &a_track, &l_track, &a_sexp,
                          &l_sexp, &n_pairs, &a_conn, &l_conn, &a_rsv, &l_rsv, &a_closed, &l_closed))
        return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    const Py_ssize_t n = PyList_Size(packets);
    if (!walk_lens_ok(n, l_sl, l_exp, l_offs, l_pair, l_space, l_track, l_conn, l_rsv, l_sexp)) return NULL;
    const Py_ssize_t n_spaces = l_sexp / 8, n_conns = l_closed;
    const uint32_t *slots = (const uint32_t *)a_sl, *offs = (const uint32_t *)a_offs, *pair = (const uint32_t *)a_pair,
                   *space = (const uint32_t *)a_space, *conn = (const uint32_t *)a_conn;
    const uint64_t *exp = (const uint64_t *)a_exp;
    PyObject *ret = NULL, *outs = NULL, *res = NULL, *deferred = NULL;
    Scratch sc = {{NULL}, 0, 0};
    WalkState ws;
    if (walk_state_init(&ws, &sc, a_sexp, l_sexp, a_closed, l_closed, n_pairs) < 0) goto done;
    for (Py_ssize_t i = 0; i < n; ++i)
        if (pair[i] >= n_pairs || (Py_ssize_t)space[i] >= n_spaces ||
            (conn[i] != WALK_NO_CONN && (Py_ssize_t)conn[i] >= n_conns)) {
            PyErr_SetString(PyExc_ValueError, "pair, space or connection index out of range");
            goto done;
        }
    /* sizes, then the launch over the session's pinned staging */
    size_t total = 0;
    for (Py_ssize_t i = 0; i < n; ++i) {
        PyObject *o = PyList_GetItem(packets, i);
        if (!PyBytes_Check(o)) {
            PyErr_SetString(PyExc_TypeError, "packets must be bytes");
            goto done;
        }
        total += (size_t)PyBytes_Size(o);
    }
    qpp_desc *desc = SCRATCH0(&sc, qpp_desc, n);
    uint64_t *out_off = SCRATCH0(&sc, uint64_t, n);
    res = PyBytes_FromStringAndSize(NULL, n * (Py_ssize_t)sizeof(qpp_result));
    outs = PyList_New(n);
    deferred = PyList_New(0);
    if (sc.failed || !res || !outs || !deferred) {
        PyErr_NoMemory();
        goto done;
    }
    uint8_t *hin = NULL, *hout = NULL;
    if (n) {
        qpp_session *s = session();
        if (!s || check_rc(qpp_session_stage(s, total ? total : 1, (uint32_t)n, &hin, &hout)) < 0) goto done;
        size_t off = 0;
        for (Py_ssize_t i = 0; i < n; ++i) {
            PyObject *o = PyList_GetItem(packets, i);
            const size_t l = (size_t)PyBytes_Size(o);
            memcpy(hin + off, PyBytes_AsString(o), l);
            qpp_desc *d = &desc[i];
            d->in_off = d->out_off = out_off[i] = off;
            d->len = (uint32_t)l;
            d->hdr_len = offs[i] > 0xffff ? 0xffff : (uint16_t)offs[i];
            d->pn = exp[i];
            d->slot = slots[i];
            off += l;
        }
        if (host_call(0, kt, desc, (uint32_t)n, hin, total, hout, total, PyBytes_AsString(res)) < 0) goto done;
    }
    {
        const ResultsWalk w = {n, slots, offs, pair, space, conn, exp, out_off, (const uint8_t *)a_track,
                               (const uint8_t *)a_rsv, hout, &ws.st, outs, deferred};
        if (results_walk(&w, (qpp_result *)PyBytes_AsString(res)) < 0) goto done;
    }
    ret = PyTuple_Pack(5, outs, res, deferred, ws.sexp, ws.closed);
done:
    walk_state_clear(&ws);
    Py_XDECREF(outs);
    Py_XDECREF(res);
    Py_XDECREF(deferred);
    scratch_free_all(&sc);
    return ret;
}

/* walk_results(slots_u32, exp_u64, offs_u32, pair_u32, space_u32, track_u8,
 *              space_exp_u64, n_pairs, conn_u32, rsv_u8, closed_u8,
 *              desc, results, dix_u32, out)
 *     -> what unprotect_walk returns
 * unprotect_walk's in-order walk over a launch that has run already
 * (receive_routed's fused route + walk + unprotect): packet i's descriptor and
 * result are desc / results [dix[i]] and its output lies at out + its
 * descriptor's out_off.  Nothing is launched.  slots[i] only says whether the
 * packet's pair has a receive key (0xffffffff: none); exp[i] is the expected
 * number the launch decoded against. */
static PyObject *py_walk_results(PyObject *m, PyObject *args)
{
    const char *a_sl, *a_exp, *a_offs, *a_pair, *a_space, *a_track, *a_sexp, *a_conn, *a_rsv, *a_closed;
    const char *a_desc, *a_res, *a_dix, *a_out;
    Py_ssize_t l_sl, l_exp, l_offs, l_pair, l_space, l_track, l_sexp, l_conn, l_rsv, l_closed;
    Py_ssize_t l_desc, l_res, l_dix, l_out;
    unsigned int n_pairs;
    if (!PyArg_ParseTuple(args, "y#y#y#y#y#y#y#Iy#y#y#y#y#y#y#", &a_sl, &l_sl, &a_exp, &l_exp, &a_offs, &l_offs, &a_pair,
                          &l_pair, &a_space, &l_space, &a_track, &l_track, &a_sexp, &l_sexp, &n_pairs, &a_conn,
                          &l_conn, &a_rsv, &l_rsv, &a_closed, &l_closed, &a_desc, &l_desc, &a_res, &l_res, &a_dix,
                          &l_dix, &a_out, &l_out))
        return NULL;
    const Py_ssize_t n = l_dix / 4, nd = l_desc / (Py_ssize_t)sizeof(qpp_desc);
    if (l_dix % 4 || l_desc % (Py_ssize_t)sizeof(qpp_desc) || l_res != nd * (Py_ssize_t)sizeof(qpp_result)) {
        PyErr_SetString(PyExc_ValueError, "dix: whole u32 items; desc and results: as many whole records");
        return NULL;
    }
    if (!walk_lens_ok(n, l_sl, l_exp, l_offs, l_pair, l_space, l_track, l_conn, l_rsv, l_sexp)) return NULL;
    const Py_ssize_t n_spaces = l_sexp / 8, n_conns = l_closed;
    const uint32_t *pair = (const uint32_t *)a_pair, *space = (const uint32_t *)a_space,
                   *conn = (const uint32_t *)a_conn, *dix = (const uint32_t *)a_dix;
    const qpp_desc *desc = (const qpp_desc *)a_desc;
    const qpp_result *rin = (const qpp_result *)a_res;
    Scratch sc = {{NULL}, 0, 0};
    WalkState ws;
    uint64_t *out_off = SCRATCH0(&sc, uint64_t, n);
    PyObject *ret = NULL;
    PyObject *res = PyBytes_FromStringAndSize(NULL, n * (Py_ssize_t)sizeof(qpp_result));
    PyObject *outs = PyList_New(n), *deferred = PyList_New(0);
    if (walk_state_init(&ws, &sc, a_sexp, l_sexp, a_closed, l_closed, n_pairs) < 0) goto done;
    if (!res || !outs || !deferred) {
        PyErr_NoMemory();
        goto done;
    }
    qpp_result *r = (qpp_result *)PyBytes_AsString(res);
    for (Py_ssize_t i = 0; i < n; ++i) {
        if (pair[i] >= n_pairs || (Py_ssize_t)space[i] >= n_spaces ||
            (conn[i] != WALK_NO_CONN && (Py_ssize_t)conn[i] >= n_conns) || (Py_ssize_t)dix[i] >= nd) {
            PyErr_SetString(PyExc_ValueError, "pair, space, connection or descriptor index out of range");
            goto done;
        }
        r[i] = rin[dix[i]];
        out_off[i] = desc[dix[i]].out_off;
        /* a success lies inside the output: header and payload are copied from there */
        if (r[i].status == QPP_S_OK && (out_off[i] > (uint64_t)l_out || r[i].out_len > (uint64_t)l_out - out_off[i] ||
                                        r[i].hdr_len > r[i].out_len)) {
            PyErr_SetString(PyExc_ValueError, "a result outside the output");
            goto done;
        }
    }
    {
        const ResultsWalk w = {n, (const uint32_t *)a_sl, (const uint32_t *)a_offs, pair, space, conn,
                               (const uint64_t *)a_exp, out_off, (const uint8_t *)a_track, (const uint8_t *)a_rsv,
                               (const uint8_t *)a_out, &ws.st, outs, deferred};
        if (results_walk(&w, r) < 0) goto done;
    }
    ret = PyTuple_Pack(5, outs, res, deferred, ws.sexp, ws.closed);
done:
    walk_state_clear(&ws);
    Py_XDECREF(outs);
    Py_XDECREF(res);
    Py_XDECREF(deferred);
    scratch_free_all(&sc);
    return ret;
}

/* ------------------------------------------ batched receive, short headers -- */

/* Identity map from object pointers to small indices (open addressing). */
typedef struct {
    const void **key;
    uint32_t *val;
    size_t cap;
} PtrMap;

static int ptrmap_init(PtrMap *m, size_t n)
{
    m->cap = 16;
    while (m->cap < 2 * n + 1) m->cap <<= 1;
    m->key = (const void **)calloc(m->cap, sizeof(void *));
    m->val = (uint32_t *)calloc(m->cap, sizeof(uint32_t));
    return m->key && m->val ? 0 : -1;
}

static void ptrmap_free(PtrMap *m)
{
    free(m->key);
    free(m->val);
}

/* index of k, or insert it with value v (returns the stored value) */
static uint32_t ptrmap_get(PtrMap *m, const void *k, uint32_t v, int *inserted)
{
    size_t h = ((uintptr_t)k >> 4) * 0x9E3779B97F4A7C15ull;
    for (size_t i = h & (m->cap - 1);; i = (i + 1) & (m->cap - 1)) {
        if (m->key[i] == k) {
            *inserted = 0;
            return m->val[i];
        }
        if (!m->key[i]) {
            m->key[i] = k;
            m->val[i] = v;
            *inserted = 1;
            return v;
        }
    }
}

/* first_of_each(items) -> the distinct first elements of the (a, b) tuples of
 * `items`, by identity, in first-seen order (the connections of a batch of
 * (connection, datagram) pairs). */
static PyObject *py_first_of_each(PyObject *m, PyObject *args)
{
    PyObject *items;
    if (!PyArg_ParseTuple(args, "O!", &PyList_Type, &items)) return NULL;
    const Py_ssize_t n = PyList_Size(items);
    PtrMap pm;
    if (ptrmap_init(&pm, 64) < 0) return PyErr_NoMemory();
    PyObject *out = PyList_New(0);
    for (Py_ssize_t i = 0; out && i < n; ++i) {
        PyObject *it = PyList_GetItem(items, i);
        PyObject *a = PyTuple_Check(it) && PyTuple_Size(it) == 2 ? PyTuple_GetItem(it, 0) : NULL;
        if (!a) {
            PyErr_SetString(PyExc_TypeError, "items must be (connection, datagram) tuples");
            Py_CLEAR(out);
            break;
        }
        int ins;
        if ((size_t)PyList_Size(out) * 2 + 2 > pm.cap) {
            /* grow: rebuild from the list */
            PtrMap g;
            if (ptrmap_init(&g, (size_t)PyList_Size(out) * 2 + 2) < 0) {
                Py_CLEAR(out);
                PyErr_NoMemory();
                break;
            }
            for (Py_ssize_t k = 0; k < PyList_Size(out); ++k) (void)ptrmap_get(&g, PyList_GetItem(out, k), (uint32_t)k, &ins);
            ptrmap_free(&pm);
            pm = g;
        }
        (void)ptrmap_get(&pm, a, (uint32_t)PyList_Size(out), &ins);
        if (ins && PyList_Append(out, a) < 0) Py_CLEAR(out);
    }
    ptrmap_free(&pm);
    return out;
}

/* A record of the caller's tuple subclass (receive.ReceivedPacket), built
 * without a Python-level call: fields are borrowed references.  A record
 * refers only to objects that cannot refer back to it (ints, bytes, None,
 * enum members), so it can never be part of a reference cycle: it is taken
 * off the cycle collector's lists, which a batch of 64 Ki records would
 * otherwise keep traversing. */
static PyObject *make_record(PyTypeObject *tp, allocfunc alloc, PyObject *const *f, int nf)
{
    PyObject *r = alloc(tp, nf);
    if (!r) return NULL;
    for (int k = 0; k < nf; ++k) {
        Py_INCREF(f[k]);
        if (PyTuple_SetItem(r, k, f[k]) < 0) {
            Py_DECREF(r);
            return NULL;
        }
    }
    PyObject_GC_UnTrack(r);
    return r;
}

/* The in-order walk after the launch of receive_short / receive_routed:
 * CryptoPair.decrypt_packet's sequential semantics (quic/crypto.py:184-192)
 * over the records of one batch, one ReceivedPacket per record or None and an
 * entry in `deferred` (the record's position) for the caller's general path.
 * Record j is datagram dg[j] (NULL: j itself) of connection conn_of[j];
 * slot_of[j] >= RS_CLOSED means nothing was launched for it; otherwise its
 * descriptor and result are desc / res [rix[j]], or, with rix NULL, the next
 * of the launched ones in order. */
typedef struct {
    Py_ssize_t n;
    const uint32_t *dg, *rix;
    const uint32_t *conn_of, *slot_of, *cpair, *cspace;
    const qpp_desc *desc;
    const qpp_result *res;
    const uint8_t *hout;
    RxWalkState *st;
    /* receive_routed_phase (NULL otherwise, as st->rolled is): qpp_route_phase's verdict per descriptor */
    const uint8_t *phase;
    PyObject *recs, *deferred;
    PyTypeObject *tp;
    allocfunc alloc;
    PyObject *ptype, *epoch;
    /* output copies: header and payload of every packet, for the caller's par_copy */
    uint8_t **od;
    const uint8_t **os_;
    size_t *ol, on, otot;
} ShortWalk;

/* the record of a datagram that yields no packet */
static PyObject *drop_record(const ShortWalk *w, PyObject *di, PyObject *epoch, PyObject *why)
{
    PyObject *f[9] = {di, g_zero, Py_None, w->ptype, epoch, g_empty, g_empty, g_minus1, why};
    return make_record(w->tp, w->alloc, f, 9);
}

static int short_walk(ShortWalk *w)
{
    uint32_t k = 0;
    for (Py_ssize_t i = 0; i < w->n; ++i) {
        const uint32_t c = w->conn_of[i];
        RxWalkPacket f = {.pair = w->cpair[c], .space = w->cspace[c], .conn = c, .launched = w->slot_of[i] < RS_CLOSED,
                          .rsv_mask = 0x18, .track = 1, .phase = RXWALK_NO_PHASE};
        const qpp_result *ri = NULL;
        const uint8_t *o = NULL;
        if (f.launched) {
            const uint32_t x = w->rix ? w->rix[i] : k++;
            ri = &w->res[x];
            o = w->hout + w->desc[x].out_off;
            f.status = ri->status, f.hdr_len = ri->hdr_len, f.pn = ri->pn;
            f.pn_off = w->desc[x].hdr_len, f.exp = w->desc[x].pn;
            if (ri->status == QPP_S_OK) f.first = o[0];
            if (w->phase) f.phase = w->phase[x];
        }
        const RxWalkVerdict v = rxwalk_step(w->st, &f);
        PyObject *di = PyLong_FromSsize_t(w->dg ? (Py_ssize_t)w->dg[i] : i);
        if (!di) return -1;
        PyObject *rec = NULL;
        if (v == RXW_DEFERRED) {
            /* the record's position, for the caller's general path */
            PyObject *dj = w->dg ? PyLong_FromSsize_t(i) : di;
            const int bad = dj ? PyList_Append(w->deferred, dj) : -1;
            if (w->dg) Py_XDECREF(dj);
            Py_DECREF(di);
            if (bad < 0) return -1;
            Py_INCREF(Py_None);
            PyList_SetItem(w->recs, i, Py_None);
            continue;
        }
        if (v == RXW_CLOSED) rec = drop_record(w, di, Py_None, g_s_closed);
        else if (v == RXW_NO_KEY) rec = drop_record(w, di, w->epoch, g_s_key);
        else if (v == RXW_RESERVED) rec = drop_record(w, di, w->epoch, g_s_rsv);
        else if (v == RXW_FAILED) rec = drop_record(w, di, w->epoch, g_s_dec);
        else {
            const size_t pll = (size_t)ri->out_len - ri->hdr_len;
            PyObject *h = PyBytes_FromStringAndSize(NULL, ri->hdr_len);
            PyObject *pl = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)pll);
            PyObject *pn = PyLong_FromUnsignedLongLong(ri->pn);
            if (h && pl && pn) {
                w->od[w->on] = (uint8_t *)PyBytes_AsString(h), w->os_[w->on] = o, w->ol[w->on++] = ri->hdr_len;
                w->od[w->on] = (uint8_t *)PyBytes_AsString(pl), w->os_[w->on] = o + ri->hdr_len, w->ol[w->on++] = pll;
                w->otot += ri->hdr_len + pll;
                PyObject *g[9] = {di, g_zero, Py_None, w->ptype, w->epoch, h, pl, pn, Py_None};
                rec = make_record(w->tp, w->alloc, g, 9);
            }
            Py_XDECREF(h);
            Py_XDECREF(pl);
            Py_XDECREF(pn);
        }
        Py_DECREF(di);
        if (!rec) return -1;
        PyList_SetItem(w->recs, i, rec);
    }
    return 0;
}

/* receive_short(table, items, conns, conn_cid_u32, conn_pair_u32,
 *               conn_space_u32, pair_slot_u32, space_exp_u64, rec_type,
 *               packet_type, epoch, conn_closed_u8)
 *     -> None | (records, deferred, space_exp after, conn_closed after)
 * receive_datagrams' steady state in one call: every datagram of `items`
 * ((connection, bytes) pairs) is a short-header 1-RTT packet running to the
 * datagram's end (RFC 9000 sec. 12.2), its encrypted offset 1 + the
 * connection's CID length.  One launch, then the in-order walk of
 * CryptoPair.decrypt_packet (quic/crypto.py:184-192) with the expected
 * packet numbers of connection.py:984-985, as unprotect_walk does, and one
 * record per datagram:
 *   (datagram, 0, None, packet_type, epoch, plain_header, payload, pn, None),
 *   or the drop: "key_unavailable" (pair_slot 0xffffffff: no receive key,
 *   crypto.py:78-79) / "payload_decrypt_error" (connection.py:936-947) /
 *   "reserved_bits" (a packet that authenticates with a reserved bit set
 *   closes its connection, connection.py:949-960, and leaves the expected
 *   number alone) / "connection_closed" (epoch None: a datagram of a closed
 *   connection, ignored by connection.py:756-757; nothing is launched for the
 *   connections closed on entry).
 * Deferred datagrams (key-phase flip, or a number that decodes differently
 * by now -- and every later one of their pair, space or connection) get None and their
 * index in `deferred`, for the caller's general path.  Returns None at once,
 * with nothing launched, if any datagram is not such a packet. */
static PyObject *py_receive_short(PyObject *m, PyObject *args)
{
    PyObject *t, *items, *conns, *rec_type, *ptype, *epoch;
    const char *a_cid, *a_pair, *a_space, *a_pslot, *a_sexp, *a_closed;
    Py_ssize_t l_cid, l_pair, l_space, l_pslot, l_sexp, l_closed;
    if (!PyArg_ParseTuple(args, "OO!O!y#y#y#y#y#OOOy#", &t, &PyList_Type, &items, &PyList_Type, &conns, &a_cid,
                          &l_cid, &a_pair, &l_pair, &a_space, &l_space, &a_pslot, &l_pslot, &a_sexp, &l_sexp,
                          &rec_type, &ptype, &epoch, &a_closed, &l_closed))
        return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    if (!PyType_Check(rec_type) || !PyType_IsSubtype((PyTypeObject *)rec_type, &PyTuple_Type)) {
        PyErr_SetString(PyExc_TypeError, "rec_type must be a tuple subclass");
        return NULL;
    }
    const Py_ssize_t n = PyList_Size(items), nc = PyList_Size(conns);
    const Py_ssize_t n_pairs = l_pslot / 4, n_spaces = l_sexp / 8;
    if (check_len(l_cid, nc, 4, "conn_cid") < 0 || check_len(l_pair, nc, 4, "conn_pair") < 0 ||
        check_len(l_space, nc, 4, "conn_space") < 0 || check_len(l_closed, nc, 1, "conn_closed") < 0)
        return NULL;
    const uint32_t *ccid = (const uint32_t *)a_cid, *cpair = (const uint32_t *)a_pair,
                   *cspace = (const uint32_t *)a_space, *pslot = (const uint32_t *)a_pslot;
    for (Py_ssize_t c = 0; c < nc; ++c)
        if ((Py_ssize_t)cpair[c] >= n_pairs || (Py_ssize_t)cspace[c] >= n_spaces) {
            PyErr_SetString(PyExc_ValueError, "pair or space index out of range");
            return NULL;
        }
    PyTypeObject *tp = (PyTypeObject *)rec_type;
    allocfunc alloc = (allocfunc)PyType_GetSlot(tp, Py_tp_alloc);
    if (!alloc) return NULL;
    /* a snapshot holding a reference to every (connection, datagram) item:
       the datagram copies below run without the GIL, while another thread
       may change the caller's list */
    items = PySequence_Tuple(items);
    if (!items) return NULL;

    PtrMap pm = {0};
    Scratch sc = {{NULL}, 0, 0};
    WalkState ws = {.sexp = NULL, .closed = NULL};
    PyObject *ret = NULL, *recs = NULL, *res = NULL, *deferred = NULL;
    int ins;
    if (ptrmap_init(&pm, (size_t)nc) < 0) goto nomem;
    for (Py_ssize_t c = 0; c < nc; ++c) (void)ptrmap_get(&pm, PyList_GetItem(conns, c), (uint32_t)c, &ins);
    uint32_t *conn_of = SCRATCH(&sc, uint32_t, n), *slot_of = SCRATCH(&sc, uint32_t, n);
    qpp_desc *desc = SCRATCH0(&sc, qpp_desc, n);
    uint8_t **cd = SCRATCH(&sc, uint8_t *, n);
    const uint8_t **cs = SCRATCH(&sc, const uint8_t *, n);
    size_t *cl = SCRATCH(&sc, size_t, n);
    /* output copies: header and payload of every packet, filled after the
       walk without the GIL (the bytes objects are not shared until returned) */
    uint8_t **od = SCRATCH(&sc, uint8_t *, 2 * n + 1);
    const uint8_t **os_ = SCRATCH(&sc, const uint8_t *, 2 * n + 1);
    size_t *ol = SCRATCH(&sc, size_t, 2 * n + 1);
    if (sc.failed) goto nomem;
    /* classify: every datagram a short header long enough for its CID */
    size_t total = 0;
    uint32_t nl = 0;  /* packets to launch */
    for (Py_ssize_t i = 0; i < n; ++i) {
        PyObject *it = PyTuple_GetItem(items, i);
        PyObject *c = PyTuple_Check(it) && PyTuple_Size(it) == 2 ? PyTuple_GetItem(it, 0) : NULL;
        PyObject *d = c ? PyTuple_GetItem(it, 1) : NULL;
        if (!d || !PyBytes_Check(d)) goto fallback;
        const int found = (int)ptrmap_get(&pm, c, 0xffffffffu, &ins);
        if (ins) goto fallback; /* a connection not in conns */
        const Py_ssize_t len = PyBytes_Size(d);
        const uint8_t *b = (const uint8_t *)PyBytes_AsString(d);
        if (len < 1 || (b[0] & 0xC0) != 0x40 || len < 1 + (Py_ssize_t)ccid[found]) goto fallback;
        conn_of[i] = (uint32_t)found;
        slot_of[i] = ((const uint8_t *)a_closed)[found] ? RS_CLOSED : pslot[cpair[found]];
        if (slot_of[i] >= RS_CLOSED) continue; /* closed on entry, or no receive key: no launch */
        qpp_desc *x = &desc[nl];
        x->in_off = x->out_off = total;
        x->len = (uint32_t)len;
        x->hdr_len = (uint16_t)(1 + ccid[found]);
        x->pn = ((const uint64_t *)a_sexp)[cspace[found]];
        x->slot = slot_of[i];
        x->rsv = (uint32_t)i; /* the datagram (host-side bookkeeping only) */
        cs[nl] = b;
        cl[nl] = (size_t)len;
        total += (size_t)len;
        ++nl;
    }
    if (walk_state_init(&ws, &sc, a_sexp, l_sexp, a_closed, l_closed, (size_t)n_pairs) < 0) goto done;
    res = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)nl * (Py_ssize_t)sizeof(qpp_result));
    recs = PyList_New(n);
    deferred = PyList_New(0);
    if (!res || !recs || !deferred) goto nomem;
    uint8_t *hin = NULL, *hout = NULL;
    if (nl) {
        qpp_session *ss = session();
        if (!ss || check_rc(qpp_session_stage(ss, total ? total : 1, nl, &hin, &hout)) < 0) goto done;
        for (uint32_t k = 0; k < nl; ++k) cd[k] = hin + desc[k].in_off;
        Py_BEGIN_ALLOW_THREADS  /* the snapshot holds every datagram */
        par_copy(cd, cs, cl, nl, total);
        Py_END_ALLOW_THREADS
        if (host_call(0, kt, desc, nl, hin, total, hout, total, PyBytes_AsString(res)) < 0) goto done;
    }
    {
        ShortWalk w = {n, NULL, NULL, conn_of, slot_of, cpair, cspace, desc, (const qpp_result *)PyBytes_AsString(res),
                       hout, &ws.st, NULL, recs, deferred, tp, alloc, ptype, epoch, od, os_, ol, 0, 0};
        if (short_walk(&w) < 0) goto done;
        Py_BEGIN_ALLOW_THREADS
        par_copy(od, os_, ol, w.on, w.otot);
        Py_END_ALLOW_THREADS
    }
    ret = PyTuple_Pack(4, recs, deferred, ws.sexp, ws.closed);
    goto done;
fallback:
    Py_INCREF(Py_None);
    ret = Py_None;
    goto done;
nomem:
    PyErr_NoMemory();
done:
    ptrmap_free(&pm);
    scratch_free_all(&sc);
    walk_state_clear(&ws);
    Py_DECREF(items);
    Py_XDECREF(recs);
    Py_XDECREF(res);
    Py_XDECREF(deferred);
    return ret;
}

/* receive_routed(table, map, cid_len, datagrams, conn_pair_u32, conn_space_u32,
 *                pair_slot_u32, space_exp_u64, conn_keyset_slot_u32, conn_space_exp_u64,
 *                rec_type, packet_type, epoch, conn_closed_u8, walk)
 *     -> (route, None, None)
 *      | (route, (records, deferred, space_exp after, conn_closed after), None)
 *      | (route, None, (long_idx, walk records, walk counts, descriptors, results, output))
 * receive_short for datagrams nobody has demultiplexed: `datagrams` is a list
 * of bytes, and the connection of each comes from the route records of one
 * qpp_session_route_unprotect call over the staged batch (its routing kernel
 * fills in every descriptor's slot and expected packet number from the
 * per-connection arrays built here: a closed or keyless connection gets
 * QPP_SLOT_NONE, and the walk tells them apart by the closed flags).  Then
 * the same in-order walk as receive_short, over the QPP_R_SHORT datagrams
 * only: records[j] is the j-th of them, its .datagram the caller's index;
 * `deferred` holds positions j.  `route` is the batch's packed qpp_route_rec.
 * With the walk's arrays given (conn_keyset_slot: QPP_KEYSETS slots per
 * connection, conn_space_exp: QPP_SPACES expected numbers; both empty: not
 * given) and walk != 0, the datagrams whose first byte has bit 7 set are
 * listed while the batch is staged, and the call is
 * qpp_session_route_walk_unprotect: the device walks their headers in the
 * same call.  If one of them belongs to a known connection, the third item
 * carries what the device found -- the listed indices, the qpp_walk_rec and
 * count arrays, all n + 3 x listed descriptors and results and the output
 * bytes -- and the caller runs policy and the in-order walk over it
 * (walk_results) without another launch.
 * No walk (None, nothing of the state consulted again) with walk == 0, or
 * when a long-header datagram belongs to a known connection and the walk's
 * arrays were not given: the caller's general path takes the batch then.
 *
 * receive_accept(the same arguments, acc_row_u32, acc_slot_u32, accept_flags)
 *     -> (route, None, None | (long_idx, walk records, walk counts, descriptors, results, output),
 *         (accept records, key material, secrets))
 * receive_routed for a server that also takes on new connections: the call
 * is qpp_session_accept_unprotect, with the candidates acc_row (rows of the
 * listed long-header datagrams, in the order this call lists them: the
 * datagrams whose first byte has bit 7 set, in batch order) and two key slots
 * each in acc_slot.  The walk's arrays must be given and walk != 0.  The
 * in-order walk is always the caller's: the third item carries what the
 * device found whenever a long-header datagram was listed.  The fourth item
 * holds the packed qpp_accept_rec, 2 x qpp_key_material and 2 x 32 secret
 * bytes of every candidate.
 *
 * receive_accept_reply(the arguments of receive_accept, reply_table, addr, rand, token_ctr, versions_u32,
 *                      reply_flags)
 *     -> (route, None, None | (...), (accept records, key material, secrets), (reply buffer, reply records))
 * receive_accept for a server that also answers what it does not accept
 * (asyncio/server.py:71-111): the call is qpp_session_accept_reply_unprotect.
 * addr holds 20 bytes per candidate (or is empty without QPP_RP_RETRY), rand
 * 16; the fifth item holds the 256 bytes and the packed qpp_reply_rec of
 * every candidate (zeros when no reply flag is set).
 *
 * receive_serve(the arguments of receive_accept_reply)
 *     -> (route, None, None | (...), (accept records, key material, secrets), (reply buffer, reply records),
 *         token records)
 * receive_accept_reply for a server in Retry mode that also validates the
 * tokens that come back (asyncio/server.py:112-120): the call is
 * qpp_session_serve_unprotect, and the sixth item holds the packed
 * qpp_token_rec of every candidate.
 *
 * receive_routed_phase(the arguments of receive_routed, pair_next_u32)
 *     -> (route, None | (records, deferred, space_exp after, conn_closed after, pair_rolled_u8), None | (...))
 * receive_routed with the peers' key updates resolved on the device: the call
 * is qpp_session_route_phase_unprotect, and pair_next names, per entry of
 * pair_slot, the slot of that pair's next key phase (the current HP key, the
 * next AEAD key, the other phase bit) or 0xffffffff.  A connection closed on
 * entry gets none.  The in-order walk then follows CryptoPair.decrypt_packet
 * (quic/crypto.py:184-192): a packet the device pointed at the next slot that
 * authenticates rolls its pair, before its reserved bits are looked at; one
 * that fails its tag is a payload_decrypt_error and rolls nothing; once a pair
 * has rolled, a packet that ran on the slot of the phase before is deferred,
 * as a QPP_S_KEY_PHASE packet is.  pair_rolled has one byte per pair_slot
 * entry: the pairs whose keys the caller must now update.  The walk's arrays
 * may be empty when no datagram starts with a long header. */
typedef struct {
    /* the 15 arguments every form takes */
    PyObject *t, *mo, *dgs, *rec_type, *ptype, *epoch;
    const char *a_pair, *a_space, *a_pslot, *a_sexp, *a_kslot, *a_kexp, *a_closed;
    Py_ssize_t l_pair, l_space, l_pslot, l_sexp, l_kslot, l_kexp, l_closed;
    unsigned int cid_len;
    int walk;
    /* the forms' tails: which were given, and what they hold */
    int phased, accept, reply, serve;
    PyObject *rt;
    const char *a_pnext, *a_arow, *a_aslot, *a_addr, *a_rand, *a_vers;
    Py_ssize_t l_pnext, l_arow, l_aslot, l_addr, l_rand, l_vers;
    unsigned int accept_flags, reply_flags;
    unsigned long long token_ctr;
    /* routed_prepare: what the arguments name, sizes, the per-connection arrays */
    qpp_keytab *kt, *reply_kt;
    qpp_cidmap *map;
    PyTypeObject *tp;
    allocfunc alloc;
    PyObject *snap;  /* a snapshot holding a reference to every datagram: the copies run without the GIL */
    Py_ssize_t n, nc, n_pairs, na;
    int can_walk;
    const uint32_t *cpair, *cspace;
    uint32_t *cslot, *cnext;
    uint64_t *cexp;
    const uint32_t *kslot;  /* the walk form's arrays: the caller's, or, phased and given none, built here */
    const uint64_t *kexp;
    /* routed_launch: the staged batch and everything the device wrote */
    uint32_t *lidx, nl;  /* datagrams whose first byte says long header: the device walks them */
    size_t nd, total;
    qpp_desc *desc;
    qpp_result *res;
    qpp_walk_rec *wrec;
    uint32_t *wn;
    uint8_t *phase, *hout;
    PyObject *route, *acc, *km, *secrets, *rbuf, *rrec, *trec;
    Scratch sc;
} Routed;

/* PyArg_ParseTuple over args[lo:hi] (what "y#" yields belongs to args' items, not to the slice) */
static int parse_slice(PyObject *args, Py_ssize_t lo, Py_ssize_t hi, const char *fmt, ...)
{
    PyObject *part = PyTuple_GetSlice(args, lo, hi);
    if (!part) return 0;
    va_list va;
    va_start(va, fmt);
    const int ok = PyArg_VaParse(part, fmt, va);
    va_end(va);
    Py_DECREF(part);
    return ok;
}

/* Checks, in the order the errors have always come, and the per-connection arrays. */
static int routed_prepare(Routed *r)
{
    r->kt = as_table(r->t);
    r->map = r->kt ? as_cidmap(r->mo) : NULL;
    if (!r->map) return -1;
    r->reply_kt = r->reply ? as_table(r->rt) : NULL;
    if (r->reply && !r->reply_kt) return -1;
    if (!PyType_Check(r->rec_type) || !PyType_IsSubtype((PyTypeObject *)r->rec_type, &PyTuple_Type)) {
        PyErr_SetString(PyExc_TypeError, "rec_type must be a tuple subclass");
        return -1;
    }
    if (r->cid_len < 1 || r->cid_len > QPP_CID_MAX) {
        PyErr_SetString(PyExc_ValueError, "cid_len must be 1..20");
        return -1;
    }
    const Py_ssize_t n = PyList_Size(r->dgs), nc = r->l_closed, n_pairs = r->l_pslot / 4, n_spaces = r->l_sexp / 8;
    r->n = n, r->nc = nc, r->n_pairs = n_pairs;
    if (check_len(r->l_pair, nc, 4, "conn_pair") < 0 || check_len(r->l_space, nc, 4, "conn_space") < 0) return -1;
    /* the walk's per-key-set and per-space arrays: both or neither */
    const int given = r->l_kslot || r->l_kexp;
    r->can_walk = given || nc == 0;
    if (r->can_walk && (check_len(r->l_kslot, nc, 4 * QPP_KEYSETS, "conn_keyset_slot") < 0 ||
                        check_len(r->l_kexp, nc, 8 * QPP_SPACES, "conn_space_exp") < 0))
        return -1;
    const uint32_t *cpair = r->cpair = (const uint32_t *)r->a_pair, *cspace = r->cspace = (const uint32_t *)r->a_space;
    for (Py_ssize_t c = 0; c < nc; ++c)
        if ((Py_ssize_t)cpair[c] >= n_pairs || (Py_ssize_t)cspace[c] >= n_spaces) {
            PyErr_SetString(PyExc_ValueError, "pair or space index out of range");
            return -1;
        }
    if (n > 0x7fffffff || nc > 0x7fffffff) {
        PyErr_SetString(PyExc_ValueError, "batch too large");
        return -1;
    }
    if (r->phased && r->l_pnext != r->l_pslot) {
        PyErr_SetString(PyExc_ValueError, "pair_next: one u32 per pair_slot entry");
        return -1;
    }
    r->na = r->l_arow / 4;
    if (r->accept && (r->l_arow % 4 || r->l_aslot != 8 * r->na || r->na > n || !r->walk || !r->can_walk)) {
        PyErr_SetString(PyExc_ValueError, "acc_row: whole u32 items, no more than datagrams; acc_slot: two u32 each; "
                                          "the walk's arrays are required");
        return -1;
    }
    if (r->reply && ((r->l_addr && r->l_addr != QPP_RP_ADDR_STRIDE * r->na) ||
                     r->l_rand != QPP_RP_RAND_STRIDE * r->na || r->l_vers % 4)) {
        PyErr_SetString(PyExc_ValueError, "addr: 20 bytes per candidate or none; rand: 16 bytes per candidate; "
                                          "versions: whole u32 items");
        return -1;
    }
    r->tp = (PyTypeObject *)r->rec_type;
    r->alloc = (allocfunc)PyType_GetSlot(r->tp, Py_tp_alloc);
    if (!r->alloc) return -1;
    r->snap = PySequence_Tuple(r->dgs);
    if (!r->snap) return -1;
    /* what the routing kernel hands a connection's datagrams: a closed or keyless one gets no slot */
    const uint8_t *closed = (const uint8_t *)r->a_closed;
    r->cslot = SCRATCH(&r->sc, uint32_t, nc);
    r->cexp = SCRATCH(&r->sc, uint64_t, nc);
    r->kslot = (const uint32_t *)r->a_kslot, r->kexp = (const uint64_t *)r->a_kexp;
    uint32_t *ks_own = NULL;
    uint64_t *ke_own = NULL;
    if (r->phased) {
        /* the next-phase slots, and the walk form's arrays when the caller gave none (no long header) */
        r->cnext = SCRATCH(&r->sc, uint32_t, nc);
        if (!given) {
            r->kslot = ks_own = SCRATCH(&r->sc, uint32_t, nc * QPP_KEYSETS);
            r->kexp = ke_own = SCRATCH0(&r->sc, uint64_t, nc * QPP_SPACES);
        }
    }
    if (r->sc.failed) return PyErr_NoMemory(), -1;
    for (Py_ssize_t c = 0; c < nc; ++c) {
        r->cslot[c] = closed[c] ? QPP_SLOT_NONE : ((const uint32_t *)r->a_pslot)[cpair[c]];
        r->cexp[c] = ((const uint64_t *)r->a_sexp)[cspace[c]];
        if (r->cnext) r->cnext[c] = closed[c] ? QPP_SLOT_NONE : ((const uint32_t *)r->a_pnext)[cpair[c]];
        if (ks_own) {
            for (int j = 0; j < QPP_KEYSETS - 1; ++j) ks_own[c * QPP_KEYSETS + j] = QPP_SLOT_NONE;
            ks_own[c * QPP_KEYSETS + QPP_KEYSETS - 1] = r->cslot[c];
            ke_own[c * QPP_SPACES + QPP_SPACES - 1] = r->cexp[c];
        }
    }
    return 0;
}

/* Stage the datagrams, list the long headers, run the form's one session call. */
static int routed_launch(Routed *r)
{
    const Py_ssize_t n = r->n, na = r->na;
    Scratch *sc = &r->sc;
    uint64_t *offs = SCRATCH(sc, uint64_t, n);
    uint32_t *lens = SCRATCH(sc, uint32_t, n);
    uint8_t **cd = SCRATCH(sc, uint8_t *, n);
    const uint8_t **cs = SCRATCH(sc, const uint8_t *, n);
    size_t *cl = SCRATCH(sc, size_t, n);
    r->lidx = SCRATCH(sc, uint32_t, n);
    if (r->phased) r->phase = SCRATCH0(sc, uint8_t, n);
    if (sc->failed) return PyErr_NoMemory(), -1;
    if (r->accept) {
        r->acc = PyBytes_FromStringAndSize(NULL, na * (Py_ssize_t)sizeof(qpp_accept_rec));
        r->km = PyBytes_FromStringAndSize(NULL, na * 2 * (Py_ssize_t)sizeof(qpp_key_material));
        r->secrets = PyBytes_FromStringAndSize(NULL, na * 64);
        if (!r->acc || !r->km || !r->secrets) return -1;
    }
    if (r->reply) {
        /* zeros when the call makes no reply (no flag, no candidate) */
        r->rbuf = PyBytes_FromStringAndSize(NULL, na * QPP_REPLY_STRIDE);
        r->rrec = PyBytes_FromStringAndSize(NULL, na * (Py_ssize_t)sizeof(qpp_reply_rec));
        if (!r->rbuf || !r->rrec) return -1;
        memset(PyBytes_AsString(r->rbuf), 0, (size_t)na * QPP_REPLY_STRIDE);
        memset(PyBytes_AsString(r->rrec), 0, (size_t)na * sizeof(qpp_reply_rec));
    }
    if (r->serve) {
        r->trec = PyBytes_FromStringAndSize(NULL, na * (Py_ssize_t)sizeof(qpp_token_rec));
        if (!r->trec) return -1;
        memset(PyBytes_AsString(r->trec), 0, (size_t)na * sizeof(qpp_token_rec));
    }
    size_t total = 0;
    uint32_t nl = 0;
    for (Py_ssize_t i = 0; i < n; ++i) {
        PyObject *d = PyTuple_GetItem(r->snap, i);
        if (!d || !PyBytes_Check(d)) {
            PyErr_SetString(PyExc_TypeError, "datagrams must be bytes");
            return -1;
        }
        const Py_ssize_t len = PyBytes_Size(d);
        if ((uint64_t)len > 0xffffffffu) {
            PyErr_SetString(PyExc_ValueError, "datagram too long");
            return -1;
        }
        offs[i] = total;
        lens[i] = (uint32_t)len;
        cs[i] = (const uint8_t *)PyBytes_AsString(d);
        cl[i] = (size_t)len;
        total += (size_t)len;
        if (r->walk && r->can_walk && len && (cs[i][0] & 0x80)) r->lidx[nl++] = (uint32_t)i;
    }
    if ((uint64_t)n + 3ull * nl > 0x7fffffffull) nl = 0;  /* past the fused call's limit: the general path */
    if (r->accept && na && !nl) {
        PyErr_SetString(PyExc_ValueError, "candidates without a listed long-header datagram");
        return -1;
    }
    const size_t nd = (size_t)n + 3 * (size_t)nl;
    r->nl = nl, r->nd = nd, r->total = total;
    r->desc = SCRATCH(sc, qpp_desc, nd);
    r->res = SCRATCH(sc, qpp_result, nd);
    r->wrec = SCRATCH0(sc, qpp_walk_rec, (size_t)(nl ? nl : 1) * QPP_WALK_MAX);
    r->wn = SCRATCH0(sc, uint32_t, nl);
    if (sc->failed) return PyErr_NoMemory(), -1;
    r->route = PyBytes_FromStringAndSize(NULL, n * (Py_ssize_t)sizeof(qpp_route_rec));
    if (!r->route) return -1;
    if (!n) return 0;
    qpp_route_rec *rr = (qpp_route_rec *)PyBytes_AsString(r->route);
    qpp_session *ss = session();
    uint8_t *hin = NULL;
    if (!ss || check_rc(qpp_session_stage(ss, total ? total : 1, (uint32_t)nd, &hin, &r->hout)) < 0) return -1;
    for (Py_ssize_t i = 0; i < n; ++i) cd[i] = hin + offs[i];
    const char *refused = NULL;
    int rc;
    Py_BEGIN_ALLOW_THREADS  /* the snapshot holds every datagram */
    par_copy(cd, cs, cl, (size_t)n, total);
    if (r->serve) {
        refused = "bad accept, reply or token arguments (those of receive_accept_reply, Retry mode not set in both "
                  "flags, or no addresses); nothing was launched";
        rc = qpp_session_serve_unprotect(
            ss, r->kt, r->map, r->cid_len, offs, lens, (uint32_t)n, hin, total, r->lidx, nl, r->kslot, r->kexp,
            (uint32_t)r->nc, 0, (const uint32_t *)r->a_arow, (const uint32_t *)r->a_aslot, (uint32_t)na,
            r->accept_flags, r->reply_kt, r->l_addr ? (const uint8_t *)r->a_addr : NULL, (const uint8_t *)r->a_rand,
            r->token_ctr, (const uint32_t *)r->a_vers, (uint32_t)(r->l_vers / 4), r->reply_flags, r->hout, total,
            r->desc, rr, r->res, r->wrec, r->wn, (qpp_accept_rec *)PyBytes_AsString(r->acc),
            (qpp_key_material *)PyBytes_AsString(r->km), (uint8_t *)PyBytes_AsString(r->secrets),
            (uint8_t *)PyBytes_AsString(r->rbuf), (qpp_reply_rec *)PyBytes_AsString(r->rrec),
            (qpp_token_rec *)PyBytes_AsString(r->trec));
    } else if (r->reply) {
        refused = "bad accept or reply arguments (those of receive_accept, a reply table of fewer than 3 slots, an "
                  "address length that is neither 6 nor 18, not 1..16 versions, an unknown reply flag, or a token "
                  "counter that wraps); nothing was launched";
        rc = qpp_session_accept_reply_unprotect(
            ss, r->kt, r->map, r->cid_len, offs, lens, (uint32_t)n, hin, total, r->lidx, nl, r->kslot, r->kexp,
            (uint32_t)r->nc, 0, (const uint32_t *)r->a_arow, (const uint32_t *)r->a_aslot, (uint32_t)na,
            r->accept_flags, r->reply_kt, r->l_addr ? (const uint8_t *)r->a_addr : NULL, (const uint8_t *)r->a_rand,
            r->token_ctr, (const uint32_t *)r->a_vers, (uint32_t)(r->l_vers / 4), r->reply_flags, r->hout, total,
            r->desc, rr, r->res, r->wrec, r->wn, (qpp_accept_rec *)PyBytes_AsString(r->acc),
            (qpp_key_material *)PyBytes_AsString(r->km), (uint8_t *)PyBytes_AsString(r->secrets),
            (uint8_t *)PyBytes_AsString(r->rbuf), (qpp_reply_rec *)PyBytes_AsString(r->rrec));
    } else if (r->accept) {
        refused = "bad accept arguments (acc_row not strictly increasing below the listed datagrams, a slot outside "
                  "the table or named twice, or an unknown flag); nothing was launched";
        rc = qpp_session_accept_unprotect(ss, r->kt, r->map, r->cid_len, offs, lens, (uint32_t)n, hin, total, r->lidx,
                                          nl, r->kslot, r->kexp, (uint32_t)r->nc, 0, (const uint32_t *)r->a_arow,
                                          (const uint32_t *)r->a_aslot, (uint32_t)na, r->accept_flags, r->hout, total,
                                          r->desc, rr, r->res, r->wrec, r->wn,
                                          (qpp_accept_rec *)PyBytes_AsString(r->acc),
                                          (qpp_key_material *)PyBytes_AsString(r->km),
                                          (uint8_t *)PyBytes_AsString(r->secrets));
    } else if (r->phased) {
        refused = "bad arguments (a next-phase slot outside the table); nothing was launched";
        rc = qpp_session_route_phase_unprotect(ss, r->kt, r->map, r->cid_len, offs, lens, (uint32_t)n, hin, total,
                                               r->lidx, nl, r->kslot, r->kexp, (uint32_t)r->nc, r->cnext, 0, r->hout,
                                               total, r->desc, rr, r->res, r->wrec, r->wn, r->phase);
    } else if (nl) {
        rc = qpp_session_route_walk_unprotect(ss, r->kt, r->map, r->cid_len, offs, lens, (uint32_t)n, hin, total,
                                              r->lidx, nl, r->kslot, r->kexp, (uint32_t)r->nc, 0, r->hout, total,
                                              r->desc, rr, r->res, r->wrec, r->wn);
    } else {
        rc = qpp_session_route_unprotect(ss, r->kt, r->map, r->cid_len, offs, lens, (uint32_t)n, hin, total, r->cslot,
                                         r->cexp, (uint32_t)r->nc, 0, r->hout, total, r->desc, rr, r->res);
    }
    Py_END_ALLOW_THREADS
    if (rc == QPP_E_ARG && refused) {
        PyErr_SetString(PyExc_ValueError, refused);
        return -1;
    }
    return check_rc(rc);
}

/* The in-order walk over the short-header datagrams of known connections, or what the caller needs to
 * run its own; then the form's result tuple. */
static PyObject *routed_result(Routed *r)
{
    const Py_ssize_t n = r->n;
    const qpp_route_rec *rr = (const qpp_route_rec *)PyBytes_AsString(r->route);
    const uint8_t *closed = (const uint8_t *)r->a_closed;
    PyObject *ret = NULL, *longs = NULL, *recs = NULL, *deferred = NULL, *rolled = NULL, *walked = NULL;
    WalkState ws = {.sexp = NULL, .closed = NULL};
    uint32_t *dg = SCRATCH(&r->sc, uint32_t, n), *conn_of = SCRATCH(&r->sc, uint32_t, n);
    uint32_t *slot_of = SCRATCH(&r->sc, uint32_t, n);
    uint8_t **od = SCRATCH(&r->sc, uint8_t *, 2 * n + 1);
    const uint8_t **os_ = SCRATCH(&r->sc, const uint8_t *, 2 * n + 1);
    size_t *ol = SCRATCH(&r->sc, size_t, 2 * n + 1);
    if (r->sc.failed) return PyErr_NoMemory();
    int walk = r->walk && !r->accept;  /* accepting: the in-order walk is the caller's */
    Py_ssize_t nr = 0;
    for (Py_ssize_t i = 0; i < n && walk; ++i) {
        if (rr[i].cls == QPP_R_LONG && rr[i].conn != QPP_CONN_NONE) walk = 0;
        if (rr[i].cls != QPP_R_SHORT) continue;
        const uint32_t c = rr[i].conn;  /* < nc: the kernel checked it */
        dg[nr] = (uint32_t)i;
        conn_of[nr] = c;
        slot_of[nr] = closed[c] ? RS_CLOSED : r->cslot[c];
        ++nr;
    }
    if (!walk) {
        /* long headers of known connections: with the device's walk of them
           (walk records, every descriptor and result, the output), or for
           the caller's general path */
        if (r->nl) {
            const Py_ssize_t nl = r->nl;
            PyObject *f[6] = {PyBytes_FromStringAndSize((const char *)r->lidx, nl * 4),
                              PyBytes_FromStringAndSize((const char *)r->wrec,
                                                        nl * QPP_WALK_MAX * (Py_ssize_t)sizeof(qpp_walk_rec)),
                              PyBytes_FromStringAndSize((const char *)r->wn, nl * 4),
                              PyBytes_FromStringAndSize((const char *)r->desc, (Py_ssize_t)(r->nd * sizeof(qpp_desc))),
                              PyBytes_FromStringAndSize((const char *)r->res, (Py_ssize_t)(r->nd * sizeof(qpp_result))),
                              PyBytes_FromStringAndSize((const char *)r->hout, (Py_ssize_t)r->total)};
            if (f[0] && f[1] && f[2] && f[3] && f[4] && f[5]) longs = PyTuple_Pack(6, f[0], f[1], f[2], f[3], f[4], f[5]);
            for (int k = 0; k < 6; ++k) Py_XDECREF(f[k]);
            if (!longs) return NULL;
        }
        PyObject *found = r->accept ? PyTuple_Pack(3, r->acc, r->km, r->secrets) : NULL;
        PyObject *sent = r->reply && found ? PyTuple_Pack(2, r->rbuf, r->rrec) : NULL;
        if (sent && r->serve)
            ret = PyTuple_Pack(6, r->route, Py_None, longs ? longs : Py_None, found, sent, r->trec);
        else if (sent) ret = PyTuple_Pack(5, r->route, Py_None, longs ? longs : Py_None, found, sent);
        else if (found && !r->reply) ret = PyTuple_Pack(4, r->route, Py_None, longs ? longs : Py_None, found);
        else if (!r->accept) ret = PyTuple_Pack(3, r->route, Py_None, longs ? longs : Py_None);
        Py_XDECREF(sent);
        Py_XDECREF(found);
        Py_XDECREF(longs);
        return ret;
    }
    recs = PyList_New(nr);
    deferred = PyList_New(0);
    if (walk_state_init(&ws, &r->sc, r->a_sexp, r->l_sexp, r->a_closed, r->l_closed, (size_t)r->n_pairs) < 0) goto done;
    if (r->phased) {
        rolled = PyBytes_FromStringAndSize(NULL, r->n_pairs);
        if (!rolled) goto done;
        ws.st.rolled = (uint8_t *)memset(PyBytes_AsString(rolled), 0, (size_t)r->n_pairs);
    }
    if (!recs || !deferred) goto done;
    {
        ShortWalk w = {nr, dg, dg, conn_of, slot_of, r->cpair, r->cspace, r->desc, r->res, r->hout, &ws.st, r->phase,
                       recs, deferred, r->tp, r->alloc, r->ptype, r->epoch, od, os_, ol, 0, 0};
        if (short_walk(&w) < 0) goto done;
        Py_BEGIN_ALLOW_THREADS
        par_copy(od, os_, ol, w.on, w.otot);
        Py_END_ALLOW_THREADS
    }
    walked = rolled ? PyTuple_Pack(5, recs, deferred, ws.sexp, ws.closed, rolled)
                    : PyTuple_Pack(4, recs, deferred, ws.sexp, ws.closed);
    if (walked) ret = PyTuple_Pack(3, r->route, walked, Py_None);
done:
    walk_state_clear(&ws);
    Py_XDECREF(walked);
    Py_XDECREF(rolled);
    Py_XDECREF(recs);
    Py_XDECREF(deferred);
    return ret;
}

/* form: 0 receive_routed, 1 receive_accept, 2 receive_routed_phase, 3 receive_accept_reply, 4 receive_serve */
static PyObject *receive_routed_impl(PyObject *args, int form)
{
    static const Py_ssize_t n_args[5] = {15, 18, 16, 24, 24};
    Routed r;
    memset(&r, 0, sizeof r);
    if (PyTuple_Size(args) != n_args[form]) {
        PyErr_Format(PyExc_TypeError, "function takes exactly %zd arguments (%zd given)", n_args[form],
                     PyTuple_Size(args));
        return NULL;
    }
    if (!parse_slice(args, 0, 15, "OOIO!y#y#y#y#y#y#OOOy#i", &r.t, &r.mo, &r.cid_len, &PyList_Type, &r.dgs, &r.a_pair,
                     &r.l_pair, &r.a_space, &r.l_space, &r.a_pslot, &r.l_pslot, &r.a_sexp, &r.l_sexp, &r.a_kslot,
                     &r.l_kslot, &r.a_kexp, &r.l_kexp, &r.rec_type, &r.ptype, &r.epoch, &r.a_closed, &r.l_closed,
                     &r.walk))
        return NULL;
    r.phased = form == 2, r.accept = form == 1 || form >= 3, r.reply = form >= 3, r.serve = form == 4;
    if (r.phased && !parse_slice(args, 15, 16, "y#", &r.a_pnext, &r.l_pnext)) return NULL;
    if (r.accept && !parse_slice(args, 15, 18, "y#y#I", &r.a_arow, &r.l_arow, &r.a_aslot, &r.l_aslot, &r.accept_flags))
        return NULL;
    if (r.reply && !parse_slice(args, 18, 24, "Oy#y#Ky#I", &r.rt, &r.a_addr, &r.l_addr, &r.a_rand, &r.l_rand,
                                &r.token_ctr, &r.a_vers, &r.l_vers, &r.reply_flags))
        return NULL;
    PyObject *ret = NULL;
    if (routed_prepare(&r) == 0 && routed_launch(&r) == 0) ret = routed_result(&r);
    scratch_free_all(&r.sc);
    Py_XDECREF(r.snap);
    Py_XDECREF(r.route);
    Py_XDECREF(r.acc);
    Py_XDECREF(r.km);
    Py_XDECREF(r.secrets);
    Py_XDECREF(r.rbuf);
    Py_XDECREF(r.rrec);
    Py_XDECREF(r.trec);
    return ret;
}

static PyObject *py_receive_routed(PyObject *m, PyObject *args) { return receive_routed_impl(args, 0); }
static PyObject *py_receive_accept(PyObject *m, PyObject *args) { return receive_routed_impl(args, 1); }
static PyObject *py_receive_routed_phase(PyObject *m, PyObject *args) { return receive_routed_impl(args, 2); }
static PyObject *py_receive_accept_reply(PyObject *m, PyObject *args) { return receive_routed_impl(args, 3); }
static PyObject *py_receive_serve(PyObject *m, PyObject *args) { return receive_routed_impl(args, 4); }

/* long_dcids(datagrams) -> None when no bytes object of the list starts with
 * a long header (first byte, bit 7), else the set of the destination CIDs of
 * those that do and carry one whole (flags, version, DCID length <= 20, DCID:
 * what qpp_route classes QPP_R_LONG).  Other items count as none. */
static PyObject *py_long_dcids(PyObject *m, PyObject *args)
{
    PyObject *dgs;
    if (!PyArg_ParseTuple(args, "O!", &PyList_Type, &dgs)) return NULL;
    const Py_ssize_t n = PyList_Size(dgs);
    PyObject *set = NULL;
    for (Py_ssize_t i = 0; i < n; ++i) {
        PyObject *d = PyList_GetItem(dgs, i);
        if (!d || !PyBytes_Check(d)) continue;
        const Py_ssize_t len = PyBytes_Size(d);
        const uint8_t *p = (const uint8_t *)PyBytes_AsString(d);
        if (len < 1 || !(p[0] & 0x80)) continue;
        if (!set && !(set = PySet_New(NULL))) return NULL;
        if (len < 6 || p[5] > QPP_CID_MAX || len < 6 + (Py_ssize_t)p[5]) continue;
        PyObject *cid = PyBytes_FromStringAndSize((const char *)p + 6, p[5]);
        if (!cid || PySet_Add(set, cid) < 0) {
            Py_XDECREF(cid);
            Py_DECREF(set);
            return NULL;
        }
        Py_DECREF(cid);
    }
    if (set) return set;
    Py_RETURN_NONE;
}

static PyObject *py_hp_mask_host(PyObject *m, PyObject *args)
{
    PyObject *t;
    const char *slots, *samples;
    Py_ssize_t slots_len, samples_len;
    if (!PyArg_ParseTuple(args, "Oy#y#", &t, &slots, &slots_len, &samples, &samples_len))
        return NULL;
    qpp_keytab *kt = as_table(t);
    if (!kt) return NULL;
    uint32_t n = (uint32_t)(slots_len / 4);
    if (samples_len != (Py_ssize_t)n * 16) {
        PyErr_SetString(PyExc_ValueError, "need 16 sample bytes per slot");
        return NULL;
    }
    qpp_session *s = session();
    if (!s) return NULL;
    PyObject *out = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)n * 16);
    if (!out) return NULL;
    uint8_t *o = (uint8_t *)PyBytes_AsString(out);
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = qpp_session_hp_mask(s, kt, (const uint32_t *)slots, (const uint8_t *)samples, n, o);
    Py_END_ALLOW_THREADS
    if (check_rc(rc) < 0) Py_CLEAR(out);
    return out;
}

static PyObject *py_device_ok(PyObject *m, PyObject *unused)
{
    return PyBool_FromLong(qpp_device_check() == QPP_OK);
}

static PyObject *py_abi(PyObject *m, PyObject *unused)
{
    return PyLong_FromLong(qpp_abi_version());
}

static PyObject *py_watchdog(PyObject *m, PyObject *unused)
{
    uint32_t v;
    Py_BEGIN_ALLOW_THREADS
    v = qpp_watchdog_count();
    Py_END_ALLOW_THREADS
    return PyLong_FromUnsignedLong(v);
}

#ifndef QPP_SOURCE_HASH
#error "build with -DQPP_SOURCE_HASH (aioquic_amd/build.py)"
#endif
/* the marker build.py reads back from the built extension */
static const char kSourceHash[] = "qpp-source-hash:" QPP_SOURCE_HASH;

static PyObject *py_source_hash(PyObject *m, PyObject *unused)
{
    return PyUnicode_FromString(kSourceHash + 16);
}

/* test hook: the receive walks' decode_pn_signed as it stands (tests/test_pn_decode.py) */
static PyObject *py_decode_pn_signed(PyObject *m, PyObject *args)
{
    unsigned long long pn, expected;
    int pn_len;
    if (!PyArg_ParseTuple(args, "KiK", &pn, &pn_len, &expected)) return NULL;
    if (pn_len < 1 || pn_len > 4) {
        PyErr_SetString(PyExc_ValueError, "pn_len must be 1..4");
        return NULL;
    }
    return PyLong_FromLongLong(decode_pn_signed(pn, pn_len, expected));
}

static PyMethodDef module_methods[] = {
    {"aead_deferred", py_aead_deferred, METH_VARARGS,
     "aead_deferred(cipher_name, key, iv) -> AEAD whose device key table is created at first use"},
    {"route_walk", py_route_walk, METH_VARARGS, "qpp_route_walk on device buffers"},
    {"route_walk_unprotect_host", py_route_walk_unprotect_host, METH_VARARGS,
     "qpp_session_route_walk_unprotect on host buffers"},
    {"route_walk_launches", py_route_walk_launches, METH_NOARGS, "qpp_route_walk_launches()"},
    {"route_accept", py_route_accept, METH_VARARGS, "qpp_route_accept on device buffers"},
    {"route_phase", py_route_phase, METH_VARARGS, "qpp_route_phase on device buffers"},
    {"route_phase_launches", py_route_phase_launches, METH_NOARGS, "qpp_route_phase_launches()"},
    {"send_fill", py_send_fill, METH_VARARGS, "qpp_send_fill on device buffers"},
    {"send_launches", py_send_launches, METH_NOARGS, "qpp_send_launches()"},
    {"send_protect_host", py_send_protect_host, METH_VARARGS, "qpp_session_send_protect on host arrays"},
    {"send_routed", py_send_routed, METH_VARARGS,
     "stage payloads, build their 1-RTT headers on the device and seal them: one bytes per datagram"},
    {"route_phase_unprotect_host", py_route_phase_unprotect_host, METH_VARARGS,
     "qpp_session_route_phase_unprotect: route, walk, resolve key phases and unprotect host buffers in one call"},
    {"receive_routed_phase", py_receive_routed_phase, METH_VARARGS,
     "receive_routed with a next-phase key slot per pair: peers' key updates resolved on the device"},
    {"route_accept_launches", py_route_accept_launches, METH_NOARGS, "qpp_route_accept_launches()"},
    {"route_reply", py_route_reply, METH_VARARGS, "qpp_route_reply on device buffers"},
    {"route_reply_launches", py_route_reply_launches, METH_NOARGS, "qpp_route_reply_launches()"},
    {"route_token", py_route_token, METH_VARARGS, "qpp_route_token on device buffers"},
    {"route_token_launches", py_route_token_launches, METH_NOARGS, "qpp_route_token_launches()"},
    {"route_accept_tokens", py_route_accept_tokens, METH_VARARGS, "qpp_route_accept_tokens on device buffers"},
    {"receive_serve", py_receive_serve, METH_VARARGS,
     "receive_accept_reply that also validates the Retry tokens that come back on the device"},
    {"receive_accept_reply", py_receive_accept_reply, METH_VARARGS,
     "receive_accept that also builds the Retry / Version Negotiation replies on the device"},
    {"receive_accept", py_receive_accept, METH_VARARGS,
     "receive_routed with the unrouted Initials among the candidates accepted on the device "
     "(qpp_session_accept_unprotect)"},
    {"long_dcids", py_long_dcids, METH_VARARGS,
     "long_dcids(datagrams) -> None, or the set of the DCIDs of the datagrams that start with a long header"},
    {"walk_results", py_walk_results, METH_VARARGS, "unprotect_walk's walk over the results of a launch that has run"},
    {"protect", py_protect, METH_VARARGS, "protect(table, desc_ptr, n, in_ptr, out_ptr, res_ptr, stream, plan=None)"},
    {"unprotect", py_unprotect, METH_VARARGS, "unprotect(table, desc_ptr, n, in_ptr, out_ptr, res_ptr, stream, plan=None)"},
    {"plan_build", py_plan_build, METH_VARARGS, "plan_build(plan, table, desc_ptr, n, stream)"},
    {"protect_host", py_protect_host, METH_VARARGS, "protect_host(table, desc, data, out_len) -> (out, results)"},
    {"unprotect_host", py_unprotect_host, METH_VARARGS, "unprotect_host(table, desc, data, out_len) -> (out, results)"},
    {"protect_into", py_protect_into, METH_VARARGS, "protect_into(table, desc_ptr, n, in_ptr, in_len, out_ptr, out_len, res_ptr)"},
    {"unprotect_into", py_unprotect_into, METH_VARARGS, "unprotect_into(table, desc_ptr, n, in_ptr, in_len, out_ptr, out_len, res_ptr)"},
    {"protect_list", py_protect_list, METH_VARARGS,
     "protect_list(table, slots_u32, pns_u64, headers, payloads) -> (wires, results)"},
    {"unprotect_list", py_unprotect_list, METH_VARARGS,
     "unprotect_list(table, slots_u32, expected_u64, packets, pn_offs_u32) -> (list of (header, payload) | None, results)"},
    {"protect_datagrams", py_protect_datagrams, METH_VARARGS,
     "protect_datagrams(table, plains, dg_u32, off_u32, hsize_u32, size_u32, pn_u64, slot_u32) -> (wires, results)"},
    {"unprotect_walk", py_unprotect_walk, METH_VARARGS,
     "unprotect_walk(table, slots_u32, exp_u64, packets, offs_u32, pair_u32, space_u32, track_u8, space_exp_u64, "
     "n_pairs, conn_u32, rsv_u8, closed_u8) -> (outcomes, results, deferred, space_exp, closed)"},
    {"first_of_each", py_first_of_each, METH_VARARGS, "first_of_each(items) -> distinct first elements, by identity"},
    {"receive_short", py_receive_short, METH_VARARGS,
     "receive_short(table, items, conns, conn_cid_u32, conn_pair_u32, conn_space_u32, pair_slot_u32, space_exp_u64, "
     "rec_type, packet_type, epoch) -> None | (records, deferred, space_exp)"},
    {"route", py_route, METH_VARARGS,
     "route(map, cid_len, off_ptr, len_ptr, n, in_ptr, slot_ptr, exp_ptr, n_conn, flags, desc_ptr, route_ptr, stream)"},
    {"route_unprotect_host", py_route_unprotect_host, METH_VARARGS,
     "route_unprotect_host(table, map, cid_len, offs_u64, lens_u32, data, conn_slot_u32, conn_expected_u64, flags, "
     "out_len) -> (out, desc, route, results)"},
    {"receive_routed", py_receive_routed, METH_VARARGS,
     "receive_routed(table, map, cid_len, datagrams, conn_pair_u32, conn_space_u32, pair_slot_u32, space_exp_u64, "
     "conn_keyset_slot_u32, conn_space_exp_u64, rec_type, packet_type, epoch, conn_closed_u8, walk) -> "
     "(route, None | (records, deferred, space_exp, closed), None | (long_idx, walk, walk_n, desc, results, out))"},
    {"hp_mask_host", py_hp_mask_host, METH_VARARGS, "hp_mask_host(table, slots_u32, samples) -> masks"},
    {"device_ok", py_device_ok, METH_NOARGS, "True when a gfx950 device is usable"},
    {"abi_version", py_abi, METH_NOARGS, "C ABI version of libquicpp"},
    {"watchdog_count", py_watchdog, METH_NOARGS, "GCM table-entry watchdog events on the current device (0 expected)"},
    {"source_hash", py_source_hash, METH_NOARGS, "hash of the native sources this module was built from"},
    {"_decode_pn_signed", py_decode_pn_signed, METH_VARARGS,
     "_decode_pn_signed(pn, pn_len, expected) -> the walks' decode of pn's low pn_len bytes (-1: negative); test hook"},
    {NULL},
};

static struct PyModuleDef moduledef = {
    PyModuleDef_HEAD_INIT, "aioquic_amd._crypto", "GPU packet protection (libquicpp binding).",
    -1, module_methods,
};

static int add_type(PyObject *m, PyType_Spec *spec, const char *name, PyObject **slot)
{
    PyObject *t = PyType_FromSpec(spec);
    if (!t) return -1;
    *slot = t;
    Py_INCREF(t);
    return PyModule_AddObject(m, name, t);
}

/* Refuse a stale build: libquicpp.so and this extension must come from the
 * same sources, and those must be the tree's current ones (when present). */
static int check_sources(void)
{
    const char *mine = kSourceHash + 16, *lib = qpp_source_hash();
    if (strcmp(mine, lib) != 0) {
        PyErr_Format(PyExc_ImportError,
                     "aioquic_amd: libquicpp.so (sources %s) and _crypto (sources %s) come from different "
                     "builds; run python -m aioquic_amd.build", lib, mine);
        return -1;
    }
    PyObject *mod = PyImport_ImportModule("aioquic_amd._srchash");
    if (!mod) return -1;
    PyObject *tree = PyObject_CallMethod(mod, "tree_hash", NULL);
    Py_DECREF(mod);
    if (!tree) return -1;
    int rc = 0;
    if (tree != Py_None && PyUnicode_CompareWithASCIIString(tree, mine) != 0) {
        if (!PyErr_Occurred())
            PyErr_Format(PyExc_ImportError,
                         "aioquic_amd: the native sources (%S) changed since _crypto was built (%s); "
                         "run python -m aioquic_amd.build", tree, mine);
        rc = -1;
    }
    Py_DECREF(tree);
    return rc;
}

PyMODINIT_FUNC PyInit__crypto(void)
{
    if (check_sources() < 0) return NULL;
    PyObject *m = PyModule_Create(&moduledef);
    if (!m) return NULL;
    g_crypto_error = PyErr_NewException("aioquic_amd._crypto.CryptoError", PyExc_ValueError, NULL);
    if (!g_crypto_error) return NULL;
    Py_INCREF(g_crypto_error);
    if (PyModule_AddObject(m, "CryptoError", g_crypto_error) < 0) return NULL;
    if (add_type(m, &AEAD_spec, "AEAD", &g_aead_type) < 0 ||
        add_type(m, &HP_spec, "HeaderProtection", &g_hp_type) < 0 ||
        add_type(m, &KT_spec, "KeyTable", &g_kt_type) < 0 ||
        add_type(m, &Plan_spec, "Plan", &g_plan_type) < 0 ||
        add_type(m, &Multi_spec, "MultiSession", &g_multi_type) < 0 ||
        add_type(m, &CidMap_spec, "CidMap", &g_cidmap_type) < 0)
        return NULL;
    g_empty = PyBytes_FromStringAndSize("", 0);
    g_minus1 = PyLong_FromLong(-1);
    g_zero = PyLong_FromLong(0);
    g_s_key = PyUnicode_FromString("key_unavailable");
    g_s_dec = PyUnicode_FromString("payload_decrypt_error");
    g_s_rsv = PyUnicode_FromString("reserved_bits");
    g_s_closed = PyUnicode_FromString("connection_closed");
    if (!g_empty || !g_minus1 || !g_zero || !g_s_key || !g_s_dec || !g_s_rsv || !g_s_closed) return NULL;
    PyModule_AddIntConstant(m, "DESC_SIZE", (long)sizeof(qpp_desc));
    PyModule_AddIntConstant(m, "RESULT_SIZE", (long)sizeof(qpp_result));
    PyModule_AddIntConstant(m, "KEY_MATERIAL_SIZE", (long)sizeof(qpp_key_material));
    PyModule_AddIntConstant(m, "CID_ENTRY_SIZE", (long)sizeof(qpp_cid_entry));
    PyModule_AddIntConstant(m, "ROUTE_SIZE", (long)sizeof(qpp_route_rec));
    return m;
}
