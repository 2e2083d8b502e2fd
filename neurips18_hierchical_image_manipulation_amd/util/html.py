"""``HTML``: the static result page of the reference's ``util/html.py`` -- an ``index.html`` in ``web_dir`` that shows the
pictures of ``web_dir/images`` in tables, one ``<h3>`` per header and one table row per ``add_images`` call.  Built from
plain strings (upstream renders it through the ``dominate`` package); all text is HTML-escaped."""
import os
from html import escape


class HTML(object):
    def __init__(self, web_dir, title, refresh=0):
        self.title = title
        self.web_dir = web_dir
        self.img_dir = os.path.join(self.web_dir, 'images')
        for d in (self.web_dir, self.img_dir):
            if not os.path.exists(d):
                os.makedirs(d)
        self.refresh = refresh
        self.body = []          # rendered blocks in call order
        self.t = None           # cells of the table opened last

    def get_image_dir(self):
        return self.img_dir

    def add_header(self, str):
        self.body.append('    <h3>%s</h3>' % escape('%s' % (str,)))

    def add_table(self, border=1):
        self.t = []
        self.body.append(('table', int(border), self.t))

    def add_images(self, ims, txts, links, width=512):
        self.add_table()
        for im, txt, link in zip(ims, txts, links):
            self.t.append(
                '        <td style="word-wrap: break-word;" halign="center" valign="top">\n'
                '          <p>\n'
                '            <a href="%s"><img style="width:%dpx" src="%s"></a><br>\n'
                '            <p>%s</p>\n'
                '          </p>\n'
                '        </td>' % (escape(os.path.join('images', link), quote=True), width,
                                   escape(os.path.join('images', im), quote=True), escape('%s' % (txt,))))

    def render(self):
        out = ['<!DOCTYPE html>', '<html>', '  <head>', '    <title>%s</title>' % escape(self.title)]
        if self.refresh > 0:
            out.append('    <meta content="%s" http-equiv="refresh">' % escape(str(self.refresh), quote=True))
        out += ['  </head>', '  <body>']
        for block in self.body:
            if isinstance(block, tuple):
                _, border, cells = block
                out.append('    <table border="%d" style="table-layout: fixed;">' % border)
                out += ['      <tr>'] + cells + ['      </tr>', '    </table>']
            else:
                out.append(block)
        out += ['  </body>', '</html>']
        return '\n'.join(out) + '\n'

    def save(self):
        with open('%s/index.html' % self.web_dir, 'wt') as f:
            f.write(self.render())
